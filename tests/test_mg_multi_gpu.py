"""Batched multigrid-preconditioned CG on the GPU (csrc/multigrid_multi.hip), through the product library: the
block application spmv_amd_precond_apply_device_multi bit for bit against spmv_amd_precond_apply_device column by column and against
the restatement's cycle, on fused (row-lds) and unfused levels, for every k; whole solves of spmv_amd_pcg_solve_device_multi bit for
bit against tests/pcg_multi_multigrid_restatement.py (x, history, count, verdict); columns that stop in different iterations, a zero
column, timers, repeatability; the handle as a single-vector one; and the refusals that need a device."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import multigrid_restatement as MG
import pcg_multi_multigrid_restatement as MM
import pcg_restatement as P
import stencil7 as S7
from bitwise import same_bits
from test_chebyshev_gpu import Guarded, stencil_random_values, ulps

pytestmark = pytest.mark.gpu

KMAX = 8


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def matrix_of(e, n):
    return MG.sorted_csr(sp.csr_matrix((e["value"], (e["row"], e["col"])), shape=(n * n, n * n)))


def interleaved(columns):
    """(k, rows) -> the block's memory: element (row, j) at [row * k + j]."""
    return np.ascontiguousarray(np.asarray(columns).T).ravel()


def column(block, k, j):
    return block.reshape(-1, k)[:, j]


def apply_multi(B, pc, op, cols):
    """The block application on the columns `cols` (k, rows) between sentinels; R must keep its bits. Returns (k, rows)."""
    k, rows = cols.shape
    block = interleaved(cols)
    dR, dZ = Guarded(B, block), Guarded(B, np.full(rows * k, np.nan))
    pc.apply_device_multi(op, k, dR.ptr, dZ.ptr)
    got = dZ.read()
    assert same_bits(dR.read(), block), "R changed"
    dR.free(), dZ.free()
    return np.stack([column(got, k, j) for j in range(k)])


def apply_single(B, pc, op, r):
    dr, dz = Guarded(B, r), Guarded(B, np.full(len(r), np.nan))
    pc.apply_device(op, dr.ptr, dz.ptr)
    z = dz.read()
    dr.free(), dz.free()
    return z


# ---------------------------------------------------------------- application, bit for bit
def check_application(B, n, A, entries, nu, max_levels, ks, label):
    B.lib().spmv_amd_reset_host_matrices()
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(entries, rows, rows, n)) == 0
    pc = B.Precond.multigrid_multi(op, nu, max_levels, KMAX)
    assert pc.kind == "multigrid" and pc.multigrid_max_rhs() == KMAX and pc.multigrid_dimension() == 2
    got_nu, grids, lmax = pc.multigrid_info()
    assert got_nu == nu and grids == MG.grids(n, max_levels)
    levels = MG.hierarchy(A, n, nu, max_levels, lambda_max=lmax)  # the library's reported bounds
    cycle = MM.make_cycle(levels)
    kmax = max(ks)
    R = np.random.default_rng(n + nu).standard_normal((kmax, rows))
    want = np.stack([cycle(R[j]) for j in range(kmax)])         # the restatement, once per column
    alone = np.stack([apply_single(B, pc, op, R[j]) for j in range(kmax)])  # the same handle, one vector at a time
    assert same_bits(alone, want), (label, "single application against the restatement")
    for k in ks:
        got = apply_multi(B, pc, op, R[:k])
        for j in range(k):
            assert same_bits(got[j], alone[j]), (label, k, j, int(np.sum(got[j] != alone[j])), float(np.max(np.abs(got[j] - alone[j]))))
            assert same_bits(got[j], want[j]), (label, k, j)
    if 1 in ks and KMAX in ks:  # slot 0 of k = 1 and slot 5 of k = 8: the same bits
        moved = apply_multi(B, pc, op, R[[3, 4, 5, 6, 7, 0, 1, 2]])
        assert same_bits(moved[5], alone[0]) and same_bits(moved[0], alone[3]), label
    variant = op.variant()
    pc.destroy()
    op.free()
    return variant


@pytest.mark.parametrize("n", [8, 9, 65, 130])
def test_application_bit_for_bit(B, monkeypatch, n):
    """nu = 0, 1, 2 with the row-lds threshold at 64 (the single path runs its fused step on every level of 64 and more, the block path
    the row-lds SpMM + the step kernel) and at its default. 8: one level; 9: two, odd; 65: odd at every level; 130: an even fine grid
    over odd ones. Every k on 130 at nu = 1; k = 1, 3, 8 elsewhere."""
    e = stencil_random_values(n)
    A = matrix_of(e, n)
    for nu in (0, 1, 2):
        ks = tuple(range(1, KMAX + 1)) if (n == 130 and nu == 1) else (1, 3, 8)
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
        variant = check_application(B, n, A, e, nu, 0, ks, f"{n} nu {nu} row-lds from 64")
        assert variant == ("stencil5/row-lds" if n >= 64 else "stencil5/row-direct")
        monkeypatch.delenv("SPMV_AMD_ROWLDS_MIN_GRID")
        variant = check_application(B, n, A, e, nu, 0, ks, f"{n} nu {nu}")
        assert variant == "stencil5/row-direct"


def test_application_on_a_row_lds_grid(B):
    """640: row-lds by itself on level 0; a bit-symmetric matrix with varying coefficients; k = 2."""
    n = 640
    A = MG.conductance_stencil(n, 7)
    assert check_application(B, n, A, P.entries_of(A), 1, 0, (2,), "conductance640 nu 1") == "stencil5/row-lds"


@pytest.mark.parametrize("max_levels", [1, 2])
def test_application_with_capped_levels(B, max_levels):
    n = 65
    e = stencil_random_values(n)
    check_application(B, n, matrix_of(e, n), e, 1, max_levels, (1, 3, 8), f"65 max_levels {max_levels}")


@pytest.mark.parametrize("kind", ["none", "jacobi", "chebyshev:3"])
def test_the_other_kinds_through_the_block_application(B, kind):
    n, k = 130, 3
    rows = n * n
    e = stencil_random_values(n)
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(e, rows, rows, n)) == 0
    pc = B.Precond.chebyshev(op, 3) if kind == "chebyshev:3" else B.Precond(op, kind)
    assert pc.multigrid_max_rhs() == 0
    R = np.random.default_rng(5).standard_normal((k, rows))
    got = apply_multi(B, pc, op, R)
    for j in range(k):
        assert same_bits(got[j], apply_single(B, pc, op, R[j])), (kind, j)
    pc.destroy()
    op.free()


# ---------------------------------------------------------------- whole solves
@functools.lru_cache(maxsize=2)
def batch_of(name):
    """A table system with k = 3 distinct right-hand sides: the table's own (b, x0), ones from zero, a random pair."""
    A, b, x0, n = MG.table_system(name)
    N = len(b)
    rng = np.random.default_rng(N + len(name))
    Bk = np.stack([b, np.ones(N), rng.standard_normal(N)])
    X0 = np.stack([x0, np.zeros(N), rng.standard_normal(N)])
    return A, P.entries_of(A), n, Bk, X0


def open_system(B, name, nu, max_rhs=KMAX):
    A, e, n, Bk, X0 = batch_of(name)
    m = B.HostMatrix(e, n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    return A, n, Bk, X0, op, m, B.Precond.multigrid_multi(op, nu, 0, max_rhs)


@pytest.mark.parametrize("name,nu,tol,iterations", MG.TABLE)
def test_whole_solves_bit_for_bit_against_the_restatement(B, name, nu, tol, iterations):
    A, n, Bk, X0, op, m, pc = open_system(B, name, nu)
    try:
        _, grids, lmax = pc.multigrid_info()
        own = MG.hierarchy(A, n, nu)
        assert max(ulps(g, L.lambda_max) for g, L in zip(lmax, own)) <= 4
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0, tol=tol)
        for j in range(len(Bk)):
            x, hist, its, converged, breakdown = MM.solve(A, n, Bk[j], X0[j], nu, tol, lambda_max=lmax)
            assert stats[j].iterations == its and stats[j].converged == int(converged) == 1 and not breakdown, (name, j, stats[j].iterations, its)
            assert same_bits(hists[j], hist), (name, nu, tol, j)
            assert same_bits(X[j], x), (name, nu, tol, j, int(np.sum(X[j] != x)))
        assert stats[0].iterations == iterations  # the table's own column
        again = B.pcg_solve_multi(op, m, pc, Bk, X0, tol=tol)  # the same solve twice: the same bits
        assert same_bits(again[0], X) and all(same_bits(a, c) for a, c in zip(again[1], hists))
    finally:
        pc.destroy()
        op.free()


def test_columns_that_stop_in_different_iterations_and_a_zero_column(B):
    """Four columns of poisson127 that stop in different iterations: each has the bits of the same column solved alone at k = 1 (so no
    launch after a column stopped moved a bit of its x, history or count, and no column's bits depend on k or its slot). Then b = 0
    beside two of them: p.Ap = 0 breaks it down in iteration 1 by the existing rule, its x stays finite, the others keep their bits."""
    A, n, Bk3, X03, op, m, pc = open_system(B, "poisson127", 1)
    try:
        N = n * n
        s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
        rng = np.random.default_rng(3)
        Bk = np.stack([Bk3[0], np.outer(s, s).ravel(), rng.standard_normal(N), 1e-3 * rng.standard_normal(N) + np.outer(s, s).ravel()])
        X0 = np.zeros_like(Bk)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        counts = [st.iterations for st in stats]
        assert all(st.converged == 1 for st in stats) and len(set(counts)) >= 2, counts
        for j in range(len(Bk)):
            x1, h1, s1 = B.pcg_solve_multi(op, m, pc, Bk[j:j + 1], X0[j:j + 1])
            assert s1[0].iterations == counts[j] and same_bits(x1[0], X[j]) and same_bits(h1[0], hists[j]), (j, counts)
        for slot in (0, 1, 2):
            mixed = np.insert(Bk[[0, 2]], slot, np.zeros(N), axis=0)
            Xm, hm, sm = B.pcg_solve_multi(op, m, pc, mixed, np.zeros((3, N)))
            assert sm[slot].converged == 0 and sm[slot].iterations == 1 and len(hm[slot]) == 2 and np.all(np.isfinite(Xm[slot])), slot
            assert np.all(Xm[slot] == 0.0)
            for at, j in zip([i for i in range(3) if i != slot], (0, 2)):
                assert same_bits(Xm[at], X[j]) and same_bits(hm[at], hists[j]) and sm[at].iterations == counts[j], (slot, j)
    finally:
        pc.destroy()
        op.free()


@pytest.mark.parametrize("rowlds_from", [64, None])
def test_detailed_timers_change_no_bit(B, monkeypatch, rowlds_from):
    if rowlds_from is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", str(rowlds_from))
    n = 130
    rows = n * n
    m = B.HostMatrix(P.entries_of(P.stencil5(n, center=4.0)), rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    assert op.variant() == ("stencil5/row-lds" if rowlds_from is not None else "stencil5/row-direct")
    pc = B.Precond.multigrid_multi(op, 1, 0, 4)
    Bk = np.random.default_rng(n).standard_normal((3, rows))
    X0 = np.zeros_like(Bk)
    plain = B.pcg_solve_multi(op, m, pc, Bk, X0)
    timed = B.pcg_solve_multi(op, m, pc, Bk, X0, timers=1)
    assert same_bits(plain[0], timed[0]) and all(same_bits(a, c) for a, c in zip(plain[1], timed[1]))
    assert [s.iterations for s in plain[2]] == [s.iterations for s in timed[2]] and all(s.converged == 1 for s in timed[2])
    t = timed[2][0]
    assert t.time_spmv_ms > 0 and t.time_blas1_ms > 0 and t.time_reductions_ms > 0
    assert t.time_spmv_ms + t.time_blas1_ms + t.time_reductions_ms <= t.time_total_ms
    assert plain[2][0].time_spmv_ms == 0 and plain[2][0].time_blas1_ms == 0 and plain[2][0].time_total_ms > 0
    pc.destroy()
    op.free()


def test_the_handle_is_a_single_vector_handle_too(B):
    """spmv_amd_pcg_solve_device and spmv_amd_precond_apply_device with the new handle against a handle of the old creator: bit for bit."""
    A, n, Bk, X0, op, m, pc = open_system(B, "poisson127", 1, max_rhs=3)
    old = B.Precond.multigrid(op, 1)
    try:
        assert pc.multigrid_max_rhs() == 3 and old.multigrid_max_rhs() == 0
        (nu_a, grids_a, lmax_a), (nu_b, grids_b, lmax_b) = pc.multigrid_info(), old.multigrid_info()
        assert nu_a == nu_b and grids_a == grids_b and same_bits(lmax_a, lmax_b) and pc.multigrid_dimension() == old.multigrid_dimension() == 2
        assert same_bits(pc.inverse_diagonal(), old.inverse_diagonal())
        for j in range(2):
            xa, ha, sa = B.pcg_solve_device(op, m, pc, Bk[j], X0[j])
            xb, hb, sb = B.pcg_solve_device(op, m, old, Bk[j], X0[j])
            assert same_bits(xa, xb) and same_bits(ha, hb) and sa.iterations == sb.iterations and sa.converged == sb.converged == 1, j
        assert same_bits(apply_single(B, pc, op, Bk[2]), apply_single(B, old, op, Bk[2]))
    finally:
        pc.destroy(), old.destroy()
        op.free()


# ---------------------------------------------------------------- refusals that need a device
def test_refusals_on_the_device(B, capfd):
    n = 40
    rows = n * n
    e = P.entries_of(P.stencil5(n, center=4.0))
    m = B.HostMatrix(e, rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    Bk, X0 = np.ones((3, rows)), np.zeros((3, rows))

    def solves(handle, k=2):
        X, hists, stats = B.pcg_solve_multi(op, m, handle, Bk[:k], X0[:k])
        assert all(s.converged == 1 for s in stats)

    def refused(handle, *words, operator=None, matrix=None, k=3):
        with pytest.raises(RuntimeError):
            B.pcg_solve_multi(operator or op, matrix or m, handle, Bk[:k], X0[:k])
        err = capfd.readouterr().err
        assert "[PCG-MULTI]" in err or "[PCG]" in err, err
        for word in words:
            assert word in err, (word, err)

    two = B.Precond.multigrid_multi(op, 1, 0, 2)
    assert two.multigrid_max_rhs() == 2
    refused(two, "[PCG-MULTI]", "nrhs = 3", "max_rhs = 2")  # above the capacity: both numbers
    dR, dZ = B.DeviceVector(3 * rows, fill=1.0), B.DeviceVector(3 * rows, fill=0.0)
    with pytest.raises(RuntimeError):
        two.apply_device_multi(op, 3, dR.ptr, dZ.ptr)
    err = capfd.readouterr().err
    assert "[PCG-MULTI]" in err and "nrhs = 3" in err and "max_rhs = 2" in err
    for r_ptr, z_ptr in ((dR.ptr, dR.ptr), (dR.ptr, dR.ptr + 16)):  # d_Z == d_R, an overlap
        with pytest.raises(RuntimeError):
            two.apply_device_multi(op, 2, r_ptr, z_ptr)
    assert "overlaps" in capfd.readouterr().err
    solves(two)

    old = B.Precond.multigrid(op, 1)  # a handle of the old creator: the sentence tests/test_pcg_multi_gpu.py holds
    refused(old, "[PCG-MULTI]", "kind 'multigrid' keeps single vectors on every level of its hierarchy", k=2)
    with pytest.raises(RuntimeError):
        old.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
    assert "single vectors" in capfd.readouterr().err
    old.destroy()
    solves(two)

    n7 = 12  # a multigrid3d handle: the 3-D hierarchy has no block vectors
    B.lib().spmv_amd_reset_host_matrices()
    m7 = B.HostMatrix(S7.coo(n7, center=7.0, off=-1.0), n7 ** 3, n7 ** 3, n7)
    op7 = B.Operator("stencil7-csr")
    assert op7.init(m7) == 0
    pc3 = B.Precond.multigrid3d(op7, 1)
    assert pc3.multigrid_max_rhs() == 0 and pc3.multigrid_dimension() == 3
    with pytest.raises(RuntimeError):
        B.pcg_solve_multi(op7, m7, pc3, np.ones((2, n7 ** 3)), np.zeros((2, n7 ** 3)))
    err = capfd.readouterr().err
    assert "[PCG-MULTI]" in err and "multigrid" in err
    with pytest.raises(ValueError) as info:  # and the block creator keeps refusing stencil7-csr
        B.Precond.multigrid_multi(op7, 1, 0, 4)
    assert info.value.bad_row == -1 and "is not stencil5-csr" in capfd.readouterr().err
    pc3.destroy()
    op7.free()
    solves(two)

    for mode in ("cusparse-csr", "ellpack"):  # initialised, but not stencil5-csr
        o = B.Operator(mode)
        assert o.init(m) == 0
        with pytest.raises(ValueError) as info:
            B.Precond.multigrid_multi(o, 1, 0, 4)
        assert info.value.bad_row == -1
        if mode == "cusparse-csr":
            refused(two, "refused", operator=o, k=2)  # a foreign handle
        o.free()
    capfd.readouterr()
    solves(two)

    assert op.init(m) == 0  # a stale one: made before the operator was last initialised
    refused(two, "refused", k=2)
    with pytest.raises(RuntimeError):
        two.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
    fresh = B.Precond.multigrid_multi(op, 1, 0, 3)
    solves(fresh, k=3)
    op.free()
    capfd.readouterr()
    refused(fresh, "[PCG-MULTI]", k=2)  # after free()
    with pytest.raises(RuntimeError):
        fresh.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
    for p in (two, fresh):
        p.destroy()
    dR.free(), dZ.free()


def _free_bytes():
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_a_zero_centre_is_refused_with_its_row_and_leaves_no_memory_behind(B):
    n = 40
    rows = n * n
    good = P.entries_of(P.stencil5(n, center=4.0))
    e = good.copy()
    at = np.nonzero((e["row"] == 777) & (e["col"] == 777))[0][0]
    e["value"][at] = 0.0
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(e, rows, rows, n)) == 0
    before = _free_bytes()
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid_multi(op, 1, 0, 8)
    assert info.value.bad_row == 777
    assert _free_bytes() >= before  # nothing of the refused hierarchy stayed on the device
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(good, rows, rows, n)
    assert op.init(m) == 0  # the operator still solves
    pc = B.Precond.multigrid_multi(op, 1, 0, 8)
    X, hists, stats = B.pcg_solve_multi(op, m, pc, np.ones((2, rows)), np.zeros((2, rows)))
    assert all(s.converged == 1 for s in stats)
    pc.destroy()
    op.free()
    # destroy() gives the block vectors back: R, D, Z, W of 8 columns on every level above 0 (a grid large enough for the allocations to
    # show in the device's free bytes)
    n = 400
    assert op.init_synthetic(n) == 0
    pc = B.Precond.multigrid_multi(op, 1, 0, 8)
    held = _free_bytes()
    pc.destroy()
    assert _free_bytes() - held >= 4 * 8 * (n // 2) ** 2 * 8
    op.free()
