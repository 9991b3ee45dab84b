"""The aggregation multigrid preconditioner of the 3-D operator (csrc/multigrid3d.hip) on the GPU: the hierarchy the
library builds bit for bit against tests/multigrid3d_restatement.py, each launch of the cycle on caller data between sentinels, the
application z = M^-1 r bit for bit with row-lds and row-direct levels, whole solves against the restatement run with the library's
reported bounds, the cycle counter, refusals and lifetime, and the application's --stencil3d --precond=multigrid."""
import math
import os
import subprocess

import numpy as np
import pytest

import multigrid3d_restatement as M3
import multigrid_restatement as MG
import pcg_restatement as P
import reduction_restatement as RR
import stencil7 as S7
from conftest import ROOT
from test_chebyshev_gpu import SUM_TOL, TOL, Guarded, timers_change_no_bit, ulps
from test_multigrid_gpu import GuardedBytes, same_bits

pytestmark = pytest.mark.gpu
ROWLDS_KNOB = "SPMV_AMD_STENCIL7_ROWLDS_MIN_GRID"
_cache = {}


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def random_values(n, seed=3):
    """The 3-D form of test_chebyshev_gpu.stencil_random_values: centres U(1, 9), every other entry U(-2, 2) (unsymmetric)."""
    e = S7.coo(n)
    u = np.random.default_rng(seed).random(len(e))
    e["value"] = np.where(e["row"] == e["col"], 1.0 + 8.0 * u, -2.0 + 4.0 * u)
    return e


def random_system(n):
    """entries, the sorted CSR and its int32 / float64 arrays: built once per n"""
    if n not in _cache:
        e = random_values(n)
        A = M3.matrix_of(e, n)
        _cache[n] = (e, A, A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data))
    return _cache[n]


def own_levels(name, A, n, max_levels=0):
    """The restatement's level matrices (nu plays no part in them): built once per system"""
    key = ("levels", name, n, max_levels)
    if key not in _cache:
        _cache[key] = M3.hierarchy(A, n, 0, max_levels)
    return _cache[key]


def with_bounds(levels, nu, lambda_max):
    """The same level matrices with the smoother of degree nu on the given bounds (multigrid3d_restatement.hierarchy's rule)."""
    out = []
    for l, L in enumerate(levels):
        last = l == len(levels) - 1
        hi = float(lambda_max[l])
        lo = hi / MG.COARSEST_RATIO if last else hi / MG.FINE_RATIO
        out.append(MG.Level(L.n, L.A, L.dinv, hi, M3.R.coefficients(MG.COARSEST_DEGREE if last else nu, lo, hi)))
    return out


def level_products(O, levels):
    """Each level's product in the operator's own order: the CSR loop (the oracle's spmv_csr)."""
    out = []
    for L in levels:
        rp, ci, va = L.A.indptr.astype(np.int32), L.A.indices.astype(np.int32), np.ascontiguousarray(L.A.data)
        out.append(lambda v, rp=rp, ci=ci, va=va: O.spmv_csr(rp, ci, va, v))
    return out


def init(B, op, m):
    B.lib().spmv_amd_reset_host_matrices()
    assert op.init(m) == 0


# ---------------------------------------------------------------- hierarchy
def test_info_and_dimension(B):
    for n, max_levels, want in ((130, 0, [130, 65, 33, 17, 9, 5]), (8, 0, [8]), (9, 0, [9, 5]), (130, 1, [130]), (130, 2, [130, 65]),
                                (130, 32, [130, 65, 33, 17, 9, 5])):
        op = B.Operator("stencil7-csr")
        assert op.init_synthetic3d(n) == 0
        pc = B.Precond.multigrid3d(op, 2, max_levels)
        assert pc.kind == "multigrid" and pc.chebyshev_info() is None and pc.multigrid_dimension() == 3
        nu, grids, lmax = pc.multigrid_info()
        assert nu == 2 and grids == want == M3.grids(n, max_levels), (n, max_levels, grids)
        assert len(lmax) == len(want) and np.all(lmax > 0.0)
        few = np.full(3, -1, dtype=np.int32)  # a short buffer gets the first `cap` grids and the full count
        assert B._pcg_lib().spmv_amd_precond_multigrid_info(pc.handle, None, None, few.ctypes.data, None, 2) == len(want)
        assert few[2] == -1 and few[0] == n
        jac = B.Precond(op, "jacobi")
        assert jac.multigrid_info() is None and jac.multigrid_dimension() == 0
        jac.destroy()
        pc.destroy()
        op.free()
    n = 40
    flat = B.Operator("stencil5-csr")  # a 2-D preconditioner reports dimension 2
    init(B, flat, B.HostMatrix(P.entries_of(P.stencil5(n, center=4.0)), n * n, n * n, n))
    pc = B.Precond.multigrid(flat, 1)
    assert pc.multigrid_dimension() == 2
    pc.destroy()
    flat.free()


@pytest.mark.parametrize("n", [9, 10, 17, 34])
def test_level_matrices_bit_for_bit(Blab, n):
    """Every level's CSR and dinv equal the restatement's bit for bit (the coarse entries' sums in the stated order), lambda_max to 4 ulp."""
    e, A, _, _, _ = random_system(n)
    op = Blab.Operator("stencil7-csr")
    init(Blab, op, Blab.HostMatrix(e, n ** 3, n ** 3, n))
    pc = Blab.Precond.multigrid3d(op, 1)
    _, grids, lmax = pc.multigrid_info()
    levels = M3.hierarchy(A, n, 1)
    assert grids == [L.n for L in levels]
    for l, L in enumerate(levels):
        rp, ci, va, dinv = pc.multigrid_level(l)
        assert len(va) == S7.nnz(L.n)
        assert np.array_equal(rp, L.A.indptr) and np.array_equal(ci, L.A.indices), (n, l)
        assert same_bits(va, L.A.data), (n, l, int(np.sum(va != L.A.data)))
        assert same_bits(dinv, L.dinv), (n, l)
        assert ulps(lmax[l], L.lambda_max) <= 4, (n, l, lmax[l], L.lambda_max)
    assert same_bits(pc.inverse_diagonal(), levels[0].dinv)
    pc.destroy()
    op.free()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- stages between sentinels
@pytest.mark.parametrize("n", [9, 10, 128, 129, 130])
def test_residual_restrict_and_prolong_stages(Blab, O, n):
    """9: one short tile, a lone last plane and grid row; 10: even; 128: whole tiles; 129: a second tile with one live column, grid
    rows 8-byte aligned only, a lone last plane and grid row; 130: a short second tile. Bit for bit against the oracle's CSR product
    and fma and the restatement's sum over the members; the inputs come back unchanged, the coarse vector starts as NaN."""
    _, A, rp, ci, va = random_system(n)
    nc = (n + 1) // 2
    rng = np.random.default_rng(n)
    z, r, ec = rng.standard_normal(n ** 3), rng.standard_normal(n ** 3), rng.standard_normal(nc ** 3)
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    dz, dr, dc = Guarded(Blab, z), Guarded(Blab, r), Guarded(Blab, np.full(nc ** 3, np.nan))
    a = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
    assert Blab.mg_stage("residual_restrict3d", a) == 0
    want = M3.restrict(O.axpy(-1.0, O.spmv_csr(rp, ci, va, z), r), n)
    got = dc.read()
    assert same_bits(got, want), (n, int(np.sum(got != want)), np.nonzero(got != want)[0][:8])
    assert same_bits(dz.read(), z) and same_bits(dr.read(), r)  # only read
    assert same_bits(d_va.read(), va) and np.array_equal(d_rp.read(), rp) and np.array_equal(d_ci.read(), ci)

    de = Guarded(Blab, ec)
    a = Blab.MgStageArgs(n=n, z=dz.ptr, coarse=de.ptr)
    assert Blab.mg_stage("prolong3d", a) == 0
    assert same_bits(dz.read(), O.axpy(2.0, M3.prolong(ec, n), z)), n
    assert same_bits(de.read(), ec)
    for g in (d_rp, d_ci, d_va, dz, dr, dc, de):
        g.free()


@pytest.mark.parametrize("n", [9, 10, 17, 34])
def test_coarsen_stage(Blab, n):
    _, A, rp, ci, va = random_system(n)
    want = M3.coarsen(A, n)
    nc = (n + 1) // 2
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    o_rp = GuardedBytes(Blab, np.full(nc ** 3 + 1, -7, dtype=np.int32))
    o_ci = GuardedBytes(Blab, np.full(want.nnz, -7, dtype=np.int32))
    o_va = GuardedBytes(Blab, np.full(want.nnz, np.nan))
    a = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, out_row_ptr=o_rp.ptr, out_col_idx=o_ci.ptr,
                         out_values=o_va.ptr)
    assert Blab.mg_stage("coarsen3d", a) == 0
    assert np.array_equal(o_rp.read(), want.indptr) and np.array_equal(o_ci.read(), want.indices), n
    assert same_bits(o_va.read(), want.data), n
    # refusals: an unknown stage, a misaligned vector, a grid outside 2..674, a CSR that is not the 7-point stencil of that grid
    assert Blab.mg_stage("smooth3d", a) != 0 and Blab.mg_stage("3d", a) != 0 and Blab.mg_stage(None, a) != 0
    bad = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=o_va.ptr + 8, r=o_va.ptr, coarse=o_va.ptr)
    assert Blab.mg_stage("residual_restrict3d", bad) != 0
    bad = Blab.MgStageArgs(n=n, z=o_va.ptr + 8, coarse=o_va.ptr)
    assert Blab.mg_stage("prolong3d", bad) != 0
    for grid in (1, 675):
        bad = Blab.MgStageArgs(n=grid, z=o_va.ptr, coarse=o_va.ptr)
        assert Blab.mg_stage("prolong3d", bad) != 0
    if n == 9:  # the arrays hold a 9^3 stencil: as an 8^3 one the structure check refuses them (8^3 rows and their entries lie inside)
        a.n = 8
        assert Blab.mg_stage("coarsen3d", a) != 0
        assert np.all(o_rp.read() == want.indptr)  # nothing was written
    for g in (d_rp, d_ci, d_va, o_rp, o_ci, o_va):
        g.free()


# ---------------------------------------------------------------- application, bit for bit
def check_application(B, O, n, A, entries, nu, max_levels, label, name):
    rows = n ** 3
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(entries, rows, rows, n))
    pc = B.Precond.multigrid3d(op, nu, max_levels)
    got_nu, grids, lmax = pc.multigrid_info()
    assert got_nu == nu and grids == M3.grids(n, max_levels)
    own = own_levels(name, A, n, max_levels)
    assert max(ulps(g, L.lambda_max) for g, L in zip(lmax, own)) <= 4, label
    levels = with_bounds(own, nu, lmax)  # the library's reported bounds
    want = M3.make_cycle(levels, level_products(O, levels), fma=O.axpy)
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


@pytest.mark.parametrize("n", [8, 9, 33, 66])
def test_application_bit_for_bit(B, O, monkeypatch, n):
    """nu = 0, 1, 2 with the row-lds threshold at its default (64: level 0 of the 66 grid is row-lds, everything else row-direct) and
    raised above 66 (row-direct everywhere): the same bits from both, and the restatement's. 8: one level; 9: two, odd; 33: odd at
    every level; 66: an even fine grid over odd ones."""
    e, A, _, _, _ = random_system(n)
    for nu in (0, 1, 2):
        monkeypatch.delenv(ROWLDS_KNOB, raising=False)
        auto, variant = check_application(B, O, n, A, e, nu, 0, f"{n}^3 nu {nu}", "random")
        assert variant == ("stencil7/row-lds" if n >= 64 else "stencil7/row-direct")
        monkeypatch.setenv(ROWLDS_KNOB, "100")
        direct, variant = check_application(B, O, n, A, e, nu, 0, f"{n}^3 nu {nu} row-lds from 100", "random")
        assert variant == "stencil7/row-direct"
        assert same_bits(auto, direct), (n, nu)


@pytest.mark.parametrize("max_levels", [1, 2])
def test_application_with_capped_levels(B, O, max_levels):
    n = 33
    e, A, _, _, _ = random_system(n)
    check_application(B, O, n, A, e, 1, max_levels, f"33^3 max_levels {max_levels}", "random")


# ---------------------------------------------------------------- whole solves
def solve_row(Bx, name, nu, tol, iterations):
    A, b, x0, n = M3.table_system(name)
    rows = n ** 3
    entries = P.entries_of(A)
    m = Bx.HostMatrix(entries, rows, rows, n)
    op = Bx.Operator("stencil7-csr")
    init(Bx, op, m)
    pc = Bx.Precond.multigrid3d(op, nu)
    _, grids, lmax = pc.multigrid_info()
    xo, ho, ito, conv = M3.pcg(A, n, b, x0, nu, tol, 1000, lambda_max=lmax)  # the restatement with the library's reported bounds
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


@pytest.mark.parametrize("name,nu,tol,iterations", M3.TABLE)
def test_whole_solves_against_the_restatement(B, name, nu, tol, iterations):
    op, m, pc, b, x0, st = solve_row(B, name, nu, tol, iterations)
    pc.destroy()
    op.free()


def test_the_converging_iteration_runs_no_cycle(Blab):
    """The LAB build counts the V-cycles of the loop: iterations - 1 for a solve that converged (none when the first iteration
    converges), max_iters for one that did not; 0 after a solve of another kind."""
    L = Blab.lib()
    op, m, pc, b, x0, st = solve_row(Blab, "poisson20", 1, 1e-6, 7)
    assert L.spmv_amd_pcg_last_multigrid_cycles() == 6
    _, _, st = Blab.pcg_solve_device(op, m, pc, b, x0, tol=1e30)
    assert st.converged == 1 and st.iterations == 1 and L.spmv_amd_pcg_last_multigrid_cycles() == 0
    x, h, st = Blab.pcg_solve_device(op, m, pc, b, x0, max_iters=4, tol=1e-12)
    assert st.converged == 0 and st.iterations == 4 and len(h) == 5 and L.spmv_amd_pcg_last_multigrid_cycles() == 4
    assert np.all(np.isfinite(x))
    jac = Blab.Precond(op, "jacobi")
    Blab.pcg_solve_device(op, m, jac, b, x0, max_iters=3)
    assert L.spmv_amd_pcg_last_multigrid_cycles() == 0
    jac.destroy()
    pc.destroy()
    op.free()


@pytest.mark.parametrize("rowlds_from", [None, 100])
def test_detailed_timers_change_no_bit(B, monkeypatch, rowlds_from):
    """nu = 1 on 66 -> 33 -> 17 -> 9 -> 5: the cycle's launches under the solve's timers, level 0 row-lds (the default threshold) and
    row-direct (the threshold raised)."""
    if rowlds_from is not None:
        monkeypatch.setenv(ROWLDS_KNOB, str(rowlds_from))
    n = 66
    op = B.Operator("stencil7-csr")
    m = B.HostMatrix(S7.coo(n, center=6.0), n ** 3, n ** 3, n)
    init(B, op, m)
    assert op.variant() == ("stencil7/row-lds" if rowlds_from is None else "stencil7/row-direct")
    pc = B.Precond.multigrid3d(op, 1)
    assert pc.multigrid_info()[1] == [66, 33, 17, 9, 5]
    b = np.random.default_rng(n).standard_normal(n ** 3)
    timers_change_no_bit(B, op, m, pc, b, np.zeros(n ** 3), f"multigrid3d 66 row-lds from {rowlds_from}")
    pc.destroy()
    op.free()


@pytest.mark.parametrize("rowlds_from", [None, 100])
def test_the_first_iteration_steps_along_the_application(B, O, monkeypatch, rowlds_from):
    """spmv_amd_precond_apply_device and the loop run the same application. From x0 = 0 with max_iters = 1 and tol = 0 the solve returns
    x = alpha p0, p0 = M^-1 b, alpha = r0.z0 / p0.A p0: x / alpha equals apply(b) to 2 ulp per entry (one rounding in the loop's
    multiply, one in the divide here). alpha itself is exact: both sums are restated bit for bit from the oracle's product -- the r.z
    partials of the last streaming step and the p.Ap partials of the operator's SpMV (row-lds or row-direct)."""
    if rowlds_from is not None:
        monkeypatch.setenv(ROWLDS_KNOB, str(rowlds_from))
    n = 66
    rows = n ** 3
    e, A, rp, ci, va = random_system(n)
    m = B.HostMatrix(e, rows, rows, n)
    op = B.Operator("stencil7-csr")
    init(B, op, m)
    lds = rowlds_from is None
    assert op.variant() == ("stencil7/row-lds" if lds else "stencil7/row-direct")
    pc = B.Precond.multigrid3d(op, 1)
    b = np.random.default_rng(7).standard_normal(rows)
    db, dz = Guarded(B, b), Guarded(B, np.full(rows, np.nan))
    pc.apply_device(op, db.ptr, dz.ptr)
    z = dz.read()
    x, h, st = B.pcg_solve_device(op, m, pc, b, np.zeros(rows), max_iters=1, tol=0.0)
    assert st.iterations == 1 and st.converged == 0 and len(h) == 2
    Az = O.spmv_csr(rp, ci, va, z)
    rz_partials = RR.stream_partials(b, z)
    pap_partials = RR.rowlds_partials(z, Az, n) if lds else RR.rowdirect_partials(z, Az, n)
    rz = RR.reduce_pcg(rz_partials, len(rz_partials), 1)[0]
    pap = RR.reduce_pcg(pap_partials, len(pap_partials), 1)[0]
    alpha = rz / pap
    err = float(np.max(np.abs(x / alpha - z) / np.spacing(np.abs(z))))
    print(f"multigrid3d row-lds from {rowlds_from}: alpha {alpha!r}, x / alpha against apply(b): {err:.2f} ulp")
    assert err <= 2.0, (rowlds_from, err)
    db.free(), dz.free()
    pc.destroy()
    op.free()


# ---------------------------------------------------------------- refusals and lifetime
def test_refusals_and_lifetime(B):
    n = 12
    rows = n ** 3
    e = S7.coo(n, center=6.0)
    m = B.HostMatrix(e, rows, rows, n)
    b = np.ones(rows)
    op, other = B.Operator("stencil7-csr"), B.Operator("cusparse-csr")
    init(B, op, m)
    init(B, other, m)
    for mode in ("cusparse-csr", "ellpack", "stencil5-csr"):  # initialised, but not stencil7-csr
        o = other if mode == "cusparse-csr" else B.Operator(mode)
        if o is not other:
            init(B, o, m)
        with pytest.raises(ValueError) as info:
            B.Precond.multigrid3d(o, 1)
        assert info.value.bad_row == -1
        if o is not other:
            o.free()
    with pytest.raises(ValueError):  # the 2-D creator keeps refusing the 3-D operator
        B.Precond.multigrid(op, 1)
    assert op.select_variant("csr-loop") == 0 and op.variant() == "stencil7/csr-loop"  # the forced CSR loop is refused
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d(op, 1)
    assert info.value.bad_row == -1
    assert op.select_variant(None) == 0
    pc = B.Precond.multigrid3d(op, 1)
    dr, dz = B.DeviceVector.from_host(b), B.DeviceVector(rows, fill=0.0)
    assert pc.apply_device(op, dr.ptr, dz.ptr) != 0.0
    for r_ptr, z_ptr in ((dr.ptr, dr.ptr), (dr.ptr, dr.ptr + 16)):  # d_z == d_r, an overlap
        with pytest.raises(RuntimeError):
            pc.apply_device(op, r_ptr, z_ptr)
    with pytest.raises(RuntimeError):  # another operator
        pc.apply_device(other, dr.ptr, dz.ptr)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(other, m, pc, b, np.zeros(rows))
    init(B, op, m)  # a stale one: made before the operator was last initialised
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
    with pytest.raises(RuntimeError):
        pc.apply_device(op, dr.ptr, dz.ptr)
    pc.destroy()
    fresh = B.Precond.multigrid3d(op, 1)
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


def test_an_incomplete_stencil_is_refused(B):
    """A 3-D matrix with one entry removed runs as stencil7/csr-loop: refused with bad_row = -1, and the operator is untouched."""
    n = 9
    e = S7.coo(n, center=6.0)
    e = np.delete(e, np.nonzero((e["row"] == 400) & (e["col"] == 401))[0][0])
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    assert op.variant() == "stencil7/csr-loop"
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d(op, 1)
    assert info.value.bad_row == -1
    got, _ = op.run_timed(np.ones(n ** 3))
    assert got.sum() == 6.0 * n ** 3 - (6 * n ** 3 - 6 * n * n) + 1.0
    op.free()


def test_a_bad_diagonal_is_refused_with_its_row(B):
    n = 12
    e = S7.coo(n, center=6.0)
    at = np.nonzero((e["row"] == 777) & (e["col"] == 777))[0][0]
    e["value"][at] = 0.0
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d(op, 1)
    assert info.value.bad_row == 777
    op.free()


def test_the_synthetic_poisson_matrix_is_the_host_one(B):
    """spmv_amd_init_stencil7_synthetic_values(n, 6, -1) builds on the device what tests/stencil7.coo(n, 6, -1) uploads: the same
    product, the same hierarchy bounds and a table row's solve bit for bit (tools/multigrid3d_bench.py measures on it)."""
    A, b, x0, n = M3.table_system("poisson20")
    rows = n ** 3
    m = B.HostMatrix(P.entries_of(A), rows, rows, n)
    got = []
    for synthetic in (False, True):
        op = B.Operator("stencil7-csr")
        if synthetic:
            assert op.init_synthetic3d(n, 6.0, -1.0) == 0
        else:
            init(B, op, m)
        assert op.variant() == "stencil7/row-direct"
        y, _ = op.run_timed(b)
        pc = B.Precond.multigrid3d(op, 1)
        x, h, st = B.pcg_solve_device(op, m, pc, b, x0)
        assert st.converged == 1 and st.iterations == 7
        got.append((y, pc.multigrid_info()[2], x, h))
        pc.destroy()
        op.free()
    for u, v in zip(*got):
        assert same_bits(u, v)
    op = B.Operator("stencil7-csr")  # the defaults stay the generator matrix: centre 7, neighbours -1
    assert op.init_synthetic3d(5) == 0
    assert op.run_timed(np.ones(125))[0].sum() == 125 + 6 * 25
    op.free()


def test_application_multigrid_flag(B):
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    for flag, tag in (("--precond=multigrid", "multigrid1"), ("--precond=multigrid:2", "multigrid2")):
        out = subprocess.run([exe, "--stencil3d=96", flag], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert f"--- Results for stencil7-csr+{tag} ---\nConverged: YES in " in out.stdout, out.stdout
    out = subprocess.run([exe, "--stencil3d=96", "--precond=multigrid:9"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "multigrid" in out.stderr
