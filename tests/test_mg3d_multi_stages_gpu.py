"""The two launches a 3-D level adds to the batched multigrid cycle (csrc/multigrid3d_multi.hip) one at a time on
caller data between sentinels, through the LAB build's spmv_amd_mg_multi_stage3d: residual + restriction and prolongation + correction
on interleaved block vectors of k columns, and a 3-D level's block product in its two kinds (csrc/stencil7_spmm.hip and "spmm/csr").
Every column equals the single-column statement bit for bit -- the oracle's CSR product and
fma, multigrid3d_restatement's sum over the members and its prolongation --, inputs keep their bits, nothing is written outside the
outputs, with every column marked done nothing is written at all, and a done column beside running ones moves no bit of theirs."""
import functools

import numpy as np
import pytest

import multigrid3d_restatement as M3
from bitwise import same_bits
from test_chebyshev_gpu import Guarded
from test_mg_multi_stages_gpu import Shifted, column, done_records, interleaved
from test_multigrid3d_gpu import random_system
from test_multigrid_gpu import GuardedBytes

pytestmark = pytest.mark.gpu

KMAX = 8
# 9: one short tile, odd n: the lone last plane and grid row, rows misaligned for odd k; 10: even n, all fast-path blocks in a short
# tile; 128: whole tiles exactly; 129: a second tile with one live column, plus the lone last plane / row; 130: a short second tile of
# two columns
CASES = [(n, k) for n in (9, 10, 129) for k in range(1, KMAX + 1)] + [(n, k) for n in (128, 130) for k in (1, 3, 4, 8)]


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


@functools.lru_cache(maxsize=1)  # the cases run grid by grid: one grid's eight columns at a time (130^3 rows x 8 x five arrays)
def fine_level(n, kmax=KMAX):
    """The random 7-point stencil of grid n as CSR (test_multigrid3d_gpu.random_system), kmax columns of z, r and e_c, and -- computed
    once, shared by every k -- the single-column results: A z, r_c = restrict(r - A z) and z' = fma(2, prolong(e_c), z)."""
    from oracle import oracle as O

    _, A, rp, ci, va = random_system(n)
    nc = (n + 1) // 2
    rng = np.random.default_rng(2000 + n)
    z, r, ec = rng.standard_normal((kmax, n ** 3)), rng.standard_normal((kmax, n ** 3)), rng.standard_normal((kmax, nc ** 3))
    az = np.stack([O.spmv_csr(rp, ci, va, z[j]) for j in range(kmax)])
    rc = np.stack([M3.restrict(O.axpy(-1.0, az[j], r[j]), n) for j in range(kmax)])
    zp = np.stack([O.axpy(2.0, M3.prolong(ec[j], n), z[j]) for j in range(kmax)])
    for a in (z, r, ec, rc, zp, az):
        a.setflags(write=False)
    return rp, ci, va, z, r, ec, rc, zp, az


def mixed_records(Blab, k, done):
    rec = (Blab.PcgMultiColumn * k)()
    for j in done:
        rec[j].done, rec[j].converged = 1, 1
    return GuardedBytes(Blab, np.frombuffer(bytes(rec), dtype=np.uint8).copy())


@pytest.mark.parametrize("n,k", CASES)
def test_residual_restrict3d_and_prolong3d(Blab, n, k):
    rp, ci, va, z, r, ec, rc, zp, az = fine_level(n)
    nc = (n + 1) // 2
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    done = done_records(Blab, k)
    some = mixed_records(Blab, k, [k // 2])  # one done column beside running ones (k = 1: the only one)
    for shift in ((0, 1) if (k % 2 == 1 and n == 9) else (0,)):  # odd k at n = 9: once more with every block vector 8 bytes off
        hold = (lambda v: Shifted(Blab, v, shift)) if shift else (lambda v: Guarded(Blab, v))
        zb, rb, eb = interleaved(z, k), interleaved(r, k), interleaved(ec, k)
        dz, dr, dc, de = hold(zb), hold(rb), hold(np.full(nc ** 3 * k, np.nan)), hold(eb)
        a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr, cols=done.ptr)
        assert Blab.mg_multi_stage3d("residual_restrict3d", k, a) == 0  # every column done: nothing is written
        assert np.all(np.isnan(dc.read())), (n, k)
        for records in (None, some.ptr) if k > 1 else (None,):
            a.cols = records
            assert Blab.mg_multi_stage3d("residual_restrict3d", k, a) == 0
            got = dc.read()
            for j in range(k):  # a done column beside running ones is computed like them, and moves no bit of theirs
                gj = column(got, k, j)
                assert same_bits(gj, rc[j]), (n, k, j, shift, records, int(np.sum(gj != rc[j])), np.nonzero(gj != rc[j])[0][:8])
        assert same_bits(dz.read(), zb) and same_bits(dr.read(), rb)  # only read
        assert same_bits(d_va.read(), va) and np.array_equal(d_rp.read(), rp) and np.array_equal(d_ci.read(), ci)

        a = Blab.MgMultiStageArgs(n=n, z=dz.ptr, coarse=de.ptr, cols=done.ptr)
        assert Blab.mg_multi_stage3d("prolong3d", k, a) == 0
        assert same_bits(dz.read(), zb), (n, k)  # every column done: z keeps its bits
        a.cols = some.ptr if k > 1 else None
        assert Blab.mg_multi_stage3d("prolong3d", k, a) == 0
        got = dz.read()
        for j in range(k):
            assert same_bits(column(got, k, j), zp[j]), (n, k, j, shift)
        assert same_bits(de.read(), eb)
        for g in (dz, dr, dc, de):
            g.free()
    for g in (d_rp, d_ci, d_va, done, some):
        g.free()


@pytest.mark.parametrize("n,k", CASES)
def test_the_block_product_in_both_kinds(Blab, n, k):
    """stencil7_spmm at the same n and k: every column the oracle's CSR product bit for bit, and the bits of spmm/csr on the same data;
    the input and the matrix keep their bits."""
    rp, ci, va, z, r, ec, rc, zp, az = fine_level(n)
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    for shift in ((0, 1) if (k % 2 == 1 and n == 9) else (0,)):
        hold = (lambda v: Shifted(Blab, v, shift)) if shift else (lambda v: Guarded(Blab, v))
        zb = interleaved(z, k)
        dz = hold(zb)
        got = {}
        for stage in ("stencil7_spmm", "spmm_csr"):
            dy = hold(np.full(n ** 3 * k, np.nan))
            a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, d=dy.ptr)
            assert Blab.mg_multi_stage3d(stage, k, a) == 0
            got[stage] = dy.read()
            dy.free()
            for j in range(k):
                gj = column(got[stage], k, j)
                assert same_bits(gj, az[j]), (stage, n, k, j, shift, int(np.sum(gj != az[j])), np.nonzero(gj != az[j])[0][:8])
        assert same_bits(got["stencil7_spmm"], got["spmm_csr"]), (n, k, shift)
        assert same_bits(dz.read(), zb)
        dz.free()
    assert same_bits(d_va.read(), va) and np.array_equal(d_rp.read(), rp) and np.array_equal(d_ci.read(), ci)
    for g in (d_rp, d_ci, d_va):
        g.free()


def test_a_csr_that_is_no_stencil_is_refused(Blab, capfd):
    n = 9
    rp, ci, va, z, r, ec, rc, zp, az = fine_level(n)
    wrong = ci.copy()
    wrong[7] += 1
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, wrong), GuardedBytes(Blab, va)
    dz, dr, dc = Guarded(Blab, interleaved(z, 2)), Guarded(Blab, interleaved(r, 2)), Guarded(Blab, np.full(125 * 2, np.nan))
    a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
    assert Blab.mg_multi_stage3d("residual_restrict3d", 2, a) != 0
    err = capfd.readouterr().err
    assert "[PCG-MULTI]" in err and "not a complete 7-point stencil" in err
    assert np.all(np.isnan(dc.read()))
    a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, d=dc.ptr)  # a product writes n^3 rows: refused before
    assert Blab.mg_multi_stage3d("stencil7_spmm", 2, a) != 0 and "not a complete 7-point stencil" in capfd.readouterr().err
    assert np.all(np.isnan(dc.read()))
    for g in (d_rp, d_ci, d_va, dz, dr, dc):
        g.free()
