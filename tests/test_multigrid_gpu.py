"""The aggregation multigrid preconditioner (csrc/multigrid.hip) on the GPU: the hierarchy the library builds bit
for bit against tests/multigrid_restatement.py, each launch of the cycle on caller data between sentinels, the application z = M^-1 r
bit for bit on fused (row-lds) and unfused levels, whole solves against the restatement run with the library's reported bounds, the
cycle counter, refusals and lifetime, and the application's --precond=multigrid."""
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import multigrid_restatement as MG
import pcg_restatement as P
import reduction_restatement as RR
from conftest import ROOT
from test_chebyshev_gpu import GUARD, SUM_TOL, TOL, Guarded, stencil_random_values, timers_change_no_bit, ulps

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def matrix_of(e, n):
    return MG.sorted_csr(sp.csr_matrix((e["value"], (e["row"], e["col"])), shape=(n * n, n * n)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


class GuardedBytes:
    """An array of any dtype on the device between sentinel bytes (8-byte granules; the payload stays 16-byte aligned)."""

    def __init__(self, B, values):
        self.B, self.dtype, self.n = B, values.dtype, len(values)
        raw = np.ascontiguousarray(values).view(np.uint8)
        self.nbytes = len(raw)
        body = (self.nbytes + 7) // 8 * 8
        host = np.full(2 * 8 * GUARD + body, 0xA5, dtype=np.uint8)
        host[8 * GUARD:8 * GUARD + self.nbytes] = raw
        self.host = host
        self.dev = B.DeviceVector(len(host) // 8)
        B.lib().spmv_amd_copy_to_device(self.dev.ptr, host.ctypes.data, host.nbytes)
        self.ptr = self.dev.ptr + 8 * GUARD

    def read(self):
        out = np.empty_like(self.host)
        self.B.lib().spmv_amd_device_synchronize()
        self.B.lib().spmv_amd_copy_to_host(out.ctypes.data, self.dev.ptr, out.nbytes)
        lo, hi = 8 * GUARD, 8 * GUARD + self.nbytes
        assert np.all(out[:lo] == 0xA5) and np.all(out[hi:] == 0xA5), "written outside the array"
        return out[lo:hi].copy().view(self.dtype)

    def free(self):
        self.dev.free()


def level_products(O, levels):
    """Each level's product in the stencil operator's own order (the oracle's), from the restatement's level matrices."""
    out = []
    for L in levels:
        rp, ci, va = L.A.indptr.astype(np.int32), L.A.indices.astype(np.int32), np.ascontiguousarray(L.A.data)
        out.append(lambda v, rp=rp, ci=ci, va=va, n=L.n: O.spmv_stencil5(rp, ci, va, v, n))
    return out


# ---------------------------------------------------------------- hierarchy
def test_info_reports_the_grids(B):
    for n, max_levels, want in ((130, 0, [130, 65, 33, 17, 9, 5]), (8, 0, [8]), (9, 0, [9, 5]), (130, 1, [130]), (130, 2, [130, 65]),
                                (130, 32, [130, 65, 33, 17, 9, 5])):
        B.lib().spmv_amd_reset_host_matrices()
        A = P.stencil5(n, center=4.0)
        op = B.Operator("stencil5-csr")
        assert op.init(B.HostMatrix(P.entries_of(A), n * n, n * n, n)) == 0
        pc = B.Precond.multigrid(op, 2, max_levels)
        assert pc.kind == "multigrid" and pc.chebyshev_info() is None
        nu, grids, lmax = pc.multigrid_info()
        assert nu == 2 and grids == want == MG.grids(n, max_levels), (n, max_levels, grids)
        assert len(lmax) == len(want) and np.all(lmax > 0.0)
        few = np.full(3, -1, dtype=np.int32)  # a short buffer gets the first `cap` grids and the full count
        assert B._pcg_lib().spmv_amd_precond_multigrid_info(pc.handle, None, None, few.ctypes.data, None, 2) == len(want)
        assert few[2] == -1 and few[0] == n
        jac = B.Precond(op, "jacobi")
        assert jac.multigrid_info() is None
        jac.destroy()
        pc.destroy()
        op.free()


@pytest.mark.parametrize("n", [9, 10, 17, 130])
def test_level_matrices_bit_for_bit(Blab, n):
    """Every level's CSR and dinv equal the restatement's bit for bit (the coarse entries' sums in the stated order), lambda_max to 4 ulp."""
    Blab.lib().spmv_amd_reset_host_matrices()
    e = stencil_random_values(n)
    op = Blab.Operator("stencil5-csr")
    assert op.init(Blab.HostMatrix(e, n * n, n * n, n)) == 0
    pc = Blab.Precond.multigrid(op, 1)
    _, grids, lmax = pc.multigrid_info()
    levels = MG.hierarchy(matrix_of(e, n), n, 1)
    assert grids == [L.n for L in levels]
    for l, L in enumerate(levels):
        rp, ci, va, dinv = pc.multigrid_level(l)
        assert np.array_equal(rp, L.A.indptr) and np.array_equal(ci, L.A.indices), (n, l)
        assert same_bits(va, L.A.data), (n, l, int(np.sum(va != L.A.data)))
        assert same_bits(dinv, L.dinv), (n, l)
        assert ulps(lmax[l], L.lambda_max) <= 4, (n, l, lmax[l], L.lambda_max)
    assert same_bits(pc.inverse_diagonal(), levels[0].dinv)
    pc.destroy()
    op.free()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- stages between sentinels
@pytest.mark.parametrize("n", [9, 128, 129, 130, 257])
def test_residual_restrict_and_prolong_stages(Blab, O, n):
    """128: whole tiles; 129: a second tile with one live column and a lone last grid row; 130: a short second tile; 257: three tiles,
    odd rows 8-byte aligned only; 9: a single short tile. Bit for bit against the oracle's product and fma."""
    e = stencil_random_values(n)
    A = matrix_of(e, n)
    nc = (n + 1) // 2
    rng = np.random.default_rng(n)
    z, r, ec = rng.standard_normal(n * n), rng.standard_normal(n * n), rng.standard_normal(nc * nc)
    rp, ci, va = A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    dz, dr, dc = Guarded(Blab, z), Guarded(Blab, r), Guarded(Blab, np.full(nc * nc, np.nan))
    a = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
    assert Blab.mg_stage("residual_restrict", a) == 0
    want = MG.restrict(O.axpy(-1.0, O.spmv_stencil5(rp, ci, va, z, n), r), n)
    got = dc.read()
    assert same_bits(got, want), (n, int(np.sum(got != want)), np.nonzero(got != want)[0][:8])
    assert same_bits(dz.read(), z) and same_bits(dr.read(), r)  # only read
    assert same_bits(d_va.read(), va) and np.array_equal(d_rp.read(), rp) and np.array_equal(d_ci.read(), ci)

    de = Guarded(Blab, ec)
    a = Blab.MgStageArgs(n=n, z=dz.ptr, coarse=de.ptr)
    assert Blab.mg_stage("prolong", a) == 0
    assert same_bits(dz.read(), O.axpy(2.0, MG.prolong(ec, n), z)), n
    assert same_bits(de.read(), ec)
    for g in (d_rp, d_ci, d_va, dz, dr, dc, de):
        g.free()


@pytest.mark.parametrize("n", [9, 10, 17, 130])
def test_coarsen_stage(Blab, n):
    e = stencil_random_values(n)
    A = matrix_of(e, n)
    want = MG.coarsen(A, n)
    nc = (n + 1) // 2
    rp, ci, va = A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    o_rp = GuardedBytes(Blab, np.full(nc * nc + 1, -7, dtype=np.int32))
    o_ci = GuardedBytes(Blab, np.full(want.nnz, -7, dtype=np.int32))
    o_va = GuardedBytes(Blab, np.full(want.nnz, np.nan))
    a = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, out_row_ptr=o_rp.ptr, out_col_idx=o_ci.ptr,
                         out_values=o_va.ptr)
    assert Blab.mg_stage("coarsen", a) == 0
    assert np.array_equal(o_rp.read(), want.indptr) and np.array_equal(o_ci.read(), want.indices), n
    assert same_bits(o_va.read(), want.data), n
    # refusals: an unknown stage, a misaligned vector
    assert Blab.mg_stage("smooth", a) != 0 and Blab.mg_stage(None, a) != 0
    bad = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=o_va.ptr + 8, r=o_va.ptr, coarse=o_va.ptr)
    assert Blab.mg_stage("residual_restrict", bad) != 0
    for g in (d_rp, d_ci, d_va, o_rp, o_ci, o_va):
        g.free()


# ---------------------------------------------------------------- application, bit for bit
def check_application(B, O, n, A, entries, nu, max_levels, label):
    B.lib().spmv_amd_reset_host_matrices()
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(entries, rows, rows, n)) == 0
    pc = B.Precond.multigrid(op, nu, max_levels)
    got_nu, grids, lmax = pc.multigrid_info()
    assert got_nu == nu and grids == MG.grids(n, max_levels)
    own = MG.hierarchy(A, n, nu, max_levels)
    assert max(ulps(g, L.lambda_max) for g, L in zip(lmax, own)) <= 4, label
    levels = MG.hierarchy(A, n, nu, max_levels, lambda_max=lmax)  # the library's reported bounds
    want = MG.make_cycle(levels, level_products(O, levels), fma=O.axpy)
    r = np.random.default_rng(n + nu).standard_normal(rows)
    z_want = want(r)
    dr, dz = Guarded(B, r), Guarded(B, np.full(rows, np.nan))
    rz = pc.apply_device(op, dr.ptr, dz.ptr)
    z = dz.read()
    assert same_bits(z, z_want), (label, int(np.sum(z != z_want)), float(np.max(np.abs(z - z_want))))
    assert same_bits(dr.read(), r), label
    terms = r * z_want
    err = abs(rz - math.fsum(terms)) / float(np.sum(np.abs(terms)))
    print(f"{label}: variant {op.variant()}, grids {grids}, r.z err {err:.2e} of sum|terms|")
    assert err <= SUM_TOL, (label, err)
    again = pc.apply_device(op, dr.ptr, dz.ptr)
    assert again == rz and same_bits(dz.read(), z), label
    variant = op.variant()
    dr.free(), dz.free()
    pc.destroy()
    op.free()
    return z, variant


@pytest.mark.parametrize("n", [8, 9, 65, 130])
def test_application_bit_for_bit(B, O, monkeypatch, n):
    """nu = 0, 1, 2 with the row-lds threshold at 64 (the fused step on every level of 64 and more) and at its default (the SpMV and
    the streaming step everywhere): the same bits from both, and the restatement's. 8: one level; 9: two, odd; 65: odd at every
    level; 130: an even fine grid over odd ones."""
    e = stencil_random_values(n)
    A = matrix_of(e, n)
    for nu in (0, 1, 2):
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
        fused, variant = check_application(B, O, n, A, e, nu, 0, f"{n} nu {nu} row-lds from 64")
        assert variant == ("stencil5/row-lds" if n >= 64 else "stencil5/row-direct")
        monkeypatch.delenv("SPMV_AMD_ROWLDS_MIN_GRID")
        plain, variant = check_application(B, O, n, A, e, nu, 0, f"{n} nu {nu}")
        assert variant == "stencil5/row-direct"
        assert same_bits(fused, plain), (n, nu)


def test_application_on_a_row_lds_grid(B, O):
    """640: row-lds by itself on levels 0 and (with the default threshold) no other; a bit-symmetric matrix with varying coefficients."""
    n = 640
    A = MG.conductance_stencil(n, 7)
    check_application(B, O, n, A, P.entries_of(A), 1, 0, "conductance640 nu 1")


@pytest.mark.parametrize("max_levels", [1, 2])
def test_application_with_capped_levels(B, O, max_levels):
    n = 65
    e = stencil_random_values(n)
    check_application(B, O, n, matrix_of(e, n), e, 1, max_levels, f"65 max_levels {max_levels}")


# ---------------------------------------------------------------- whole solves
def solve_row(Bx, name, nu, tol, iterations):
    A, b, x0, n = MG.table_system(name)
    rows = n * n
    entries = P.entries_of(A)
    m = Bx.HostMatrix(entries, rows, rows, n)
    op = Bx.Operator("stencil5-csr")
    assert op.init(m) == 0
    pc = Bx.Precond.multigrid(op, nu)
    _, grids, lmax = pc.multigrid_info()
    xo, ho, ito, conv = MG.pcg(A, n, b, x0, nu, tol, 1000, lambda_max=lmax)  # the restatement with the library's reported bounds
    assert conv and ito == iterations, (name, nu, tol, ito)
    x, h, st = Bx.pcg_solve_device(op, m, pc, b, x0, tol=tol)
    err = P.hist_err(h, ho) if len(h) == len(ho) else float("inf")
    print(f"{name} nu {nu} tol {tol}: {st.iterations} iterations, history {err:.2e}, x {np.max(np.abs(x - xo)) / np.max(np.abs(xo)):.2e}")
    assert st.converged == 1 and st.iterations == iterations, (name, nu, tol, st.iterations)
    assert len(h) == iterations + 1 and err < TOL, (name, nu, tol, err)
    assert np.max(np.abs(x - xo)) <= 1e-8 * np.max(np.abs(xo)), name
    assert P.true_residual_norm(entries, b, x) < tol * h[0] * (1.0 + 1e-6), name
    x2, h2, _ = Bx.pcg_solve_device(op, m, pc, b, x0, tol=tol)
    assert np.array_equal(x2, x) and np.array_equal(h2, h), name  # fixed-shape sums: the same bits
    return op, m, pc, b, x0, st


@pytest.mark.parametrize("name,nu,tol,iterations", MG.TABLE)
def test_whole_solves_against_the_restatement(B, name, nu, tol, iterations):
    op, m, pc, b, x0, st = solve_row(B, name, nu, tol, iterations)
    pc.destroy()
    op.free()


def test_the_converging_iteration_runs_no_cycle(Blab):
    """The LAB build counts the V-cycles of the loop: iterations - 1 for a solve that converged (none when the first iteration
    converges), max_iters for one that did not; 0 after a solve of another kind."""
    L = Blab.lib()
    op, m, pc, b, x0, st = solve_row(Blab, "poisson127", 1, 1e-6, 10)
    assert L.spmv_amd_pcg_last_multigrid_cycles() == 9
    _, _, st = Blab.pcg_solve_device(op, m, pc, b, x0, tol=1e30)
    assert st.converged == 1 and st.iterations == 1 and L.spmv_amd_pcg_last_multigrid_cycles() == 0
    x, h, st = Blab.pcg_solve_device(op, m, pc, b, x0, max_iters=4, tol=1e-12)
    assert st.converged == 0 and st.iterations == 4 and len(h) == 5 and L.spmv_amd_pcg_last_multigrid_cycles() == 4
    assert np.all(np.isfinite(x))
    x, h, st = Blab.pcg_solve_device(op, m, pc, b, x0, tol=1e-6, timers=1)  # detailed timers: the cycle's launches land in the breakdown
    assert st.converged == 1 and st.iterations == 10 and st.time_spmv_ms > 0.0 and st.time_blas1_ms > 0.0
    jac = Blab.Precond(op, "jacobi")
    Blab.pcg_solve_device(op, m, jac, b, x0, max_iters=3)
    assert L.spmv_amd_pcg_last_multigrid_cycles() == 0
    jac.destroy()
    pc.destroy()
    op.free()


@pytest.mark.parametrize("rowlds_from", [64, None])
def test_detailed_timers_change_no_bit(B, monkeypatch, rowlds_from):
    """nu = 1 on 130 -> 65 -> 33 -> ...: the cycle's launches under the solve's timers, with the fused step on the levels of 64 and
    more (the row-lds threshold lowered to 64) and with the SpMV + the streaming step on every level (the default threshold)."""
    if rowlds_from is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", str(rowlds_from))
    n = 130
    rows = n * n
    A = P.stencil5(n, center=4.0)
    m = B.HostMatrix(P.entries_of(A), rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    assert op.variant() == ("stencil5/row-lds" if rowlds_from is not None else "stencil5/row-direct")
    pc = B.Precond.multigrid(op, 1)
    assert pc.multigrid_info()[1] == [130, 65, 33, 17, 9, 5]
    b = np.random.default_rng(n).standard_normal(rows)
    timers_change_no_bit(B, op, m, pc, b, np.zeros(rows), f"multigrid 130 row-lds from {rowlds_from}")
    pc.destroy()
    op.free()


# ---------------------------------------------------------------- the application and the loop
@pytest.mark.parametrize("rowlds_from", [64, None])
@pytest.mark.parametrize("kind", ["chebyshev:3", "multigrid:1"])
def test_the_first_iteration_steps_along_the_application(B, O, monkeypatch, kind, rowlds_from):
    """spmv_amd_precond_apply_device and the loop run the same application. From x0 = 0 with max_iters = 1 and tol = 0 the solve
    returns x = alpha p0, p0 = M^-1 b, alpha = r0.z0 / p0.A p0: x / alpha equals apply(b) to 2 ulp per entry (one rounding in the
    loop's multiply, one in the divide here). alpha itself is exact: both sums are restated bit for bit from the oracle's product
    (tests/reduction_restatement.py) -- the r.z partials of the last step (the fused launch's slots on a row-lds plan, the streaming
    step's elsewhere) and the p.Ap partials of the operator's SpMV."""
    if rowlds_from is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", str(rowlds_from))
    n = 130
    rows = n * n
    e = stencil_random_values(n)
    rp, ci, va = O.build_csr(e, rows)
    m = B.HostMatrix(e, rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    fused = rowlds_from is not None
    assert op.variant() == ("stencil5/row-lds" if fused else "stencil5/row-direct")
    name, arg = kind.split(":")
    pc = B.Precond.chebyshev(op, int(arg)) if name == "chebyshev" else B.Precond.multigrid(op, int(arg))
    b = np.random.default_rng(7).standard_normal(rows)
    db, dz = Guarded(B, b), Guarded(B, np.full(rows, np.nan))
    pc.apply_device(op, db.ptr, dz.ptr)
    z = dz.read()
    x, h, st = B.pcg_solve_device(op, m, pc, b, np.zeros(rows), max_iters=1, tol=0.0)
    assert st.iterations == 1 and st.converged == 0 and len(h) == 2
    Az = O.spmv_stencil5(rp, ci, va, z, n)
    rz_partials = RR.rowlds_partials(b, z, n) if fused else RR.stream_partials(b, z)
    pap_partials = RR.rowlds_partials(z, Az, n) if fused else RR.rowdirect_partials(z, Az, n)
    rz = RR.reduce_pcg(rz_partials, len(rz_partials), 1)[0]
    pap = RR.reduce_pcg(pap_partials, len(pap_partials), 1)[0]
    alpha = rz / pap
    err = float(np.max(np.abs(x / alpha - z) / np.spacing(np.abs(z))))
    print(f"{kind} row-lds from {rowlds_from}: alpha {alpha!r}, x / alpha against apply(b): {err:.2f} ulp")
    assert err <= 2.0, (kind, rowlds_from, err)
    db.free(), dz.free()
    pc.destroy()
    op.free()


# ---------------------------------------------------------------- refusals and lifetime
def test_refusals_and_lifetime(B):
    n = 40
    rows = n * n
    A = P.stencil5(n, center=4.0)
    e = P.entries_of(A)
    m = B.HostMatrix(e, rows, rows, n)
    b = np.ones(rows)
    op, other = B.Operator("stencil5-csr"), B.Operator("cusparse-csr")
    assert op.init(m) == 0 and other.init(m) == 0
    for mode in ("cusparse-csr", "ellpack"):  # initialised, but not stencil5-csr
        B.lib().spmv_amd_reset_host_matrices()
        o = other if mode == "cusparse-csr" else B.Operator(mode)
        if o is not other:
            assert o.init(m) == 0
        with pytest.raises(ValueError) as info:
            B.Precond.multigrid(o, 1)
        assert info.value.bad_row == -1
        if o is not other:
            o.free()
    pc = B.Precond.multigrid(op, 1)
    dr, dz = B.DeviceVector.from_host(b), B.DeviceVector(rows, fill=0.0)
    assert pc.apply_device(op, dr.ptr, dz.ptr) != 0.0
    for r_ptr, z_ptr in ((dr.ptr, dr.ptr), (dr.ptr, dr.ptr + 16)):  # d_z == d_r, an overlap
        with pytest.raises(RuntimeError):
            pc.apply_device(op, r_ptr, z_ptr)
    with pytest.raises(RuntimeError):  # another operator
        pc.apply_device(other, dr.ptr, dz.ptr)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(other, m, pc, b, np.zeros(rows))
    assert op.init(m) == 0  # a stale one: made before the operator was last initialised
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
    with pytest.raises(RuntimeError):
        pc.apply_device(op, dr.ptr, dz.ptr)
    pc.destroy()
    fresh = B.Precond.multigrid(op, 1)
    _, _, st = B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
    assert st.converged == 1
    op.free()
    with pytest.raises(RuntimeError):  # after free()
        fresh.apply_device(op, dr.ptr, dz.ptr)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
    fresh.destroy()
    other.free()
    dr.free(), dz.free()


def test_a_bad_diagonal_is_refused_with_its_row(B):
    """Level 0: a zero centre. A coarse level: stencil_random_values(65, seed 4) has aggregates whose inner couplings outweigh their
    centres -- the first such row of level 1 comes back."""
    n = 40
    e = P.entries_of(P.stencil5(n, center=4.0))
    at = np.nonzero((e["row"] == 777) & (e["col"] == 777))[0][0]
    e["value"][at] = 0.0
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(e, n * n, n * n, n)) == 0
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid(op, 1)
    assert info.value.bad_row == 777
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
    n = 65
    e = stencil_random_values(n, seed=4)
    d1 = MG.coarsen(matrix_of(e, n), n).diagonal()
    bad_rows = np.nonzero(~((d1 != 0.0) & np.isfinite(d1) & ((d1 > 0.0) == (d1[0] > 0.0))))[0]
    assert len(bad_rows) > 0
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(e, n * n, n * n, n)) == 0
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid(op, 1)
    assert info.value.bad_row == int(bad_rows[0])
    pc = B.Precond.multigrid(op, 1, 1)  # one level: the coarse operator is never built
    pc.destroy()
    op.free()


def test_application_multigrid_flag(B):
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    for flag, tag in (("--precond=multigrid", "multigrid1"), ("--precond=multigrid:2", "multigrid2")):
        out = subprocess.run([exe, "--stencil=512", flag], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert f"--- Results for stencil5-csr+{tag} ---\nConverged: YES in " in out.stdout, out.stdout
    out = subprocess.run([exe, "--stencil=512", "--precond=multigrid:9"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "multigrid" in out.stderr
