"""Every dot-product reduction of the CG solvers, bit for bit against its numpy restatement (tests/reduction_restatement.py,
held against math.fsum by tests/test_reduction_restatement.py). The 1e-13 bounds of tests/test_blas1_gpu.py,
tests/test_pcg_stages_gpu.py and tests/test_multi_rhs_stages_gpu.py say that a sum is A correct sum; these say WHICH one: a
re-shaped tree, a partial in another slot, extras in front of the slice sums, a multiply-then-add where the kernel documents an
fma or a sum that no longer starts at +0.0 changes bits here and nowhere else. Comparisons are on bit patterns throughout."""
import ctypes as C

import numpy as np
import pytest

import reduction_restatement as R
import test_multi_rhs_stages_gpu as MS
import test_pcg_stages_gpu as PS
from bitwise import same_bits

pytestmark = pytest.mark.gpu

# 131 072: 1024 partials, the last n of the one-workgroup sum; 131 074 / 131 075: 1025 partials, the first two-stage count, without
# and with the odd tail; 1 000 001: 7813 partials, slice 31 x 253 workgroups
DOT_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097, 131_072, 131_074, 131_075, 1_000_001]
STEP_SIZES = [1, 2, 65, 129, 4097, 131_075, 1_000_001]
MULTI_COUNTS = [1, 1024, 1025, 2813, 4097, 8193]  # the batched solver's slice is 4096 partials: 4097 and 8193 take two and three


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)


def dev(B, a):
    return B.DeviceVector.from_host(a)


@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_is_the_restated_sum(B, n):
    rng = np.random.default_rng(300 + n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    partials = R.dot_partials(x, y)
    assert len(partials) == R.stream_count(n)
    dx, dy = dev(B, x), dev(B, y)
    got = C.c_double()
    assert B.lib().spmv_amd_blas1_dot(n, dx.ptr, dy.ptr, C.byref(got)) == 0
    assert same_bits(got.value, R.reduce(partials)), (got.value, R.reduce(partials))
    assert B.lib().spmv_amd_blas1_dot(n, dx.ptr, dx.ptr, C.byref(got)) == 0
    assert same_bits(got.value, R.reduce(R.dot_partials(x, x)))
    dx.free(), dy.free()


@pytest.mark.parametrize("n", STEP_SIZES)
def test_fused_slab_steps_leave_the_restated_sum(B, O, n):
    """cg_update_r_kernel (which = 0; `reverse` relabels the workgroups and must not move a partial) and
    cg_init_residual_kernel (which = 2): r.r of the r they wrote."""
    rng = np.random.default_rng(11 * n)
    Ap, r, b = (rng.standard_normal(n) for _ in range(3))
    rr_old, pAp = 3.25, 7.5
    sc = (C.c_double * 3)(rr_old, pAp, 0.3125)
    L = B.lib()
    dot = C.c_double()
    want_r = O.axpy(-(rr_old / pAp), Ap, r)
    want = R.reduce(R.residual_partials(want_r))
    for reverse in (0, 1):
        dA, dr = dev(B, Ap), dev(B, r)
        assert L.spmv_amd_cg_fused_step(0, n, sc, dA.ptr, dr.ptr, None, reverse, C.byref(dot)) == 0
        assert same_bits(dr.to_host(), want_r) and same_bits(dot.value, want), reverse
        dA.free(), dr.free()
    db, dA, drp = dev(B, b), dev(B, Ap), B.DeviceVector(2 * n, fill=0.0)
    assert L.spmv_amd_cg_fused_step(2, n, sc, db.ptr, dA.ptr, drp.ptr, 0, C.byref(dot)) == 0
    want0 = O.axpy(-1.0, Ap, b)
    assert same_bits(drp.to_host()[:n], want0) and same_bits(dot.value, R.reduce(R.residual_partials(want0)))
    for v in (db, dA, drp):
        v.free()


# ---------------------------------------------------------------- the preconditioned solver's stages (LAB build)
@pytest.mark.parametrize("kind", PS.KINDS)
@pytest.mark.parametrize("n", PS.SIZES)
def test_pcg_init_and_update_r_partials(Blab, O, n, kind):
    """The two-value partials [r.r | r.z] of pcg_init_kernel and pcg_update_r_kernel, every slot, and their two totals."""
    (b, Ap, r, _), dinv = PS.vectors(n, kind, 1)
    count = PS.partial_count(n)
    alpha = float(np.random.default_rng(n).uniform(-2.0, 2.0))
    dA, dd = PS.Guarded(Blab, Ap), PS.Guarded(Blab, dinv)
    dinv_ptr = None if kind == "none" else dd.ptr
    cases = [("init", b, O.axpy(-1.0, Ap, b), None), ("update_r", r, O.axpy(-alpha, Ap, r), Blab.PcgScalars(alpha=alpha)),
             ("update_r", r, r, Blab.PcgScalars(alpha=alpha, skip_update=1))]
    for stage, start, want_r, sc in cases:
        want_z = PS.z_of(kind, dinv, want_r)
        dstart, dpart = PS.Guarded(Blab, start), PS.Guarded(Blab, np.full(2 * count, np.nan))
        dr_out, dp_out = PS.Guarded(Blab, np.full(n, np.nan)), PS.Guarded(Blab, np.full(n, np.nan))
        if stage == "init":  # b in, r and p out
            a = Blab.PcgStageArgs(n=n, b=dstart.ptr, Ap=dA.ptr, dinv=dinv_ptr, r=dr_out.ptr, p=dp_out.ptr, partials=dpart.ptr)
        else:                # r in place
            a = Blab.PcgStageArgs(n=n, Ap=dA.ptr, dinv=dinv_ptr, r=dstart.ptr, partials=dpart.ptr)
        assert Blab.pcg_stage(stage, PS.kind_name(kind), a, sc) == 0 and a.count == count
        assert same_bits((dr_out if stage == "init" else dstart).read(), want_r), stage
        want_partials = R.stream_partials_two(want_r, want_z)
        assert same_bits(dpart.read(), want_partials), (stage, sc is not None and sc.skip_update)
        b_norm, rz = PS.two_sums(Blab, dpart.ptr, count)
        total = R.reduce_pcg(want_partials, count, 2)
        assert same_bits(b_norm, np.sqrt(np.float64(total[0]))) and same_bits(rz, total[1]), stage
        for v in (dstart, dpart, dr_out, dp_out):
            v.free()
    dA.free(), dd.free()


@pytest.mark.parametrize("count", PS.COUNTS)
def test_pcg_reduction_totals(Blab, count):
    rng = np.random.default_rng(count)
    v0, v1, vs = rng.standard_normal(count) ** 2, rng.standard_normal(count), rng.standard_normal(count)
    one = PS.Guarded(Blab, np.concatenate([vs, np.full(count, np.nan)]))
    got = PS.reduce_stage(Blab, one.ptr, count, 1, Blab.PcgScalars(rz=1.0)).pAp
    assert same_bits(got, R.reduce_pcg(vs, count, 1)[0])
    two = PS.Guarded(Blab, np.concatenate([v0, v1]))
    b_norm, rz = PS.two_sums(Blab, two.ptr, count)
    total = R.reduce_pcg(np.concatenate([v0, v1]), count, 2)
    assert same_bits(b_norm, np.sqrt(np.float64(total[0]))) and same_bits(rz, total[1])
    sc = PS.reduce_stage(Blab, two.ptr, count, 2, Blab.PcgScalars(rz=1.0, b_norm=1.0), tol=0.0)
    assert same_bits(sc.residual, np.sqrt(np.float64(total[0]))) and same_bits(sc.beta, total[1])
    one.free(), two.free()


# ---------------------------------------------------------------- the batched solver's reduce stage (LAB build)
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("count", MULTI_COUNTS)
def test_multi_rhs_reduction_totals(Blab, count, k):
    ids = [(s + 5) % 8 for s in range(k)]
    partials = np.stack([MS.partials_of(count, c) for c in ids])
    got = MS.totals(Blab, k, partials)
    for s in range(k):
        assert same_bits(got[s], R.reduce_multi(partials[s])), s
