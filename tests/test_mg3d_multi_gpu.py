"""Batched multigrid-preconditioned CG on the 3-D operator on the GPU (csrc/multigrid3d_multi.hip and the cycle of
csrc/multigrid_multi.hip), through the product library: the block application
spmv_amd_precond_apply_device_multi bit for bit against spmv_amd_precond_apply_device column by column and against the restatement's
cycle; whole solves of spmv_amd_pcg_solve_device_multi bit for bit against tests/pcg_multi_multigrid3d_restatement.py (x, history,
count, verdict); the level product at its default and forced each way (LAB build); columns that stop in different iterations, a zero column, timers, repeatability; a 64^3 system device against device;
the handle as a single-vector one; and the refusals and the lifetime that need a device."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import multigrid3d_restatement as M3
import pcg_multi_multigrid3d_restatement as MM3
import pcg_restatement as P
import stencil7 as S7
from bitwise import same_bits
from test_chebyshev_gpu import ulps
from test_mg_multi_gpu import apply_multi, apply_single
from test_multigrid3d_gpu import own_levels, random_system, with_bounds

pytestmark = pytest.mark.gpu

KMAX = 8
ROWS = [row for row in M3.TABLE if int(re.sub(r"\D", "", row[0])) <= 33]


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def open_operator(B, entries, n):
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(entries, n ** 3, n ** 3, n)
    op = B.Operator("stencil7-csr")
    assert op.init(m) == 0
    return op, m


# ---------------------------------------------------------------- application, bit for bit
def check_application(B, n, nu, max_levels, ks, label):
    e, A, _, _, _ = random_system(n)
    rows = n ** 3
    op, m = open_operator(B, e, n)
    assert op.spmm_variant() == "spmm/csr"  # the operator's own plan stays what it was
    pc = B.Precond.multigrid3d_multi(op, nu, max_levels, KMAX)
    assert pc.kind == "multigrid" and pc.multigrid_max_rhs() == KMAX and pc.multigrid_dimension() == 3
    got_nu, grids, lmax = pc.multigrid_info()
    assert got_nu == nu and grids == M3.grids(n, max_levels)
    kmax = max(ks)
    R = np.random.default_rng(n + nu).standard_normal((kmax, rows))
    alone = np.stack([apply_single(B, pc, op, R[j]) for j in range(kmax)])  # the same handle, one vector at a time
    cycle = MM3.make_cycle(with_bounds(own_levels("random", A, n, max_levels), nu, lmax))  # the library's reported bounds
    assert same_bits(alone[0], cycle(R[0])), (label, "single application against the restatement")
    for k in ks:
        got = apply_multi(B, pc, op, R[:k])
        for j in range(k):
            assert same_bits(got[j], alone[j]), (label, k, j, int(np.sum(got[j] != alone[j])), float(np.max(np.abs(got[j] - alone[j]))))
    if 1 in ks and KMAX in ks:  # slot 0 of k = 1 and slot 5 of k = 8: the same bits
        moved = apply_multi(B, pc, op, R[[3, 4, 5, 6, 7, 0, 1, 2]])
        assert same_bits(moved[5], alone[0]) and same_bits(moved[0], alone[3]), label
    pc.destroy()
    op.free()


@pytest.mark.parametrize("n", [8, 9, 33, 66])
def test_application_bit_for_bit(B, n):
    """nu = 0, 1, 2. 8: one level; 9: two, odd; 33: odd at every level; 66: an even fine grid over odd ones, level 0 of the single
    path row-lds (the block path runs spmm/csr on every level below the threshold grid of 256). Every k on 33 at nu = 1; k = 1, 3, 8 elsewhere."""
    for nu in (0, 1, 2):
        ks = tuple(range(1, KMAX + 1)) if (n == 33 and nu == 1) else (1, 3, 8)
        check_application(B, n, nu, 0, ks, f"{n}^3 nu {nu}")


@pytest.mark.parametrize("max_levels", [1, 2])
def test_application_with_capped_levels(B, max_levels):
    check_application(B, 33, 1, max_levels, (1, 3, 8), f"33^3 max_levels {max_levels}")


def test_the_level_product_at_its_default_and_forced_each_way(Blab):
    """66 -> 33 -> 17 -> 9 -> 5: by default every level is below the threshold grid of 256 and takes spmm/csr (the default above the
    threshold: test_the_default_level_product_on_a_large_grid); the LAB build forces either kind on every level, the new kernel then runs grids down to 5^3 where every grid row but
    3 x 3 lies on a face. The block application has the single application's bits under all three, and a whole solve of a table row
    with the new kernel on every level has the restatement's."""
    n, nu = 66, 1
    e, A, _, _, _ = random_system(n)
    want = {"auto": ["spmm/csr"] * 5, "csr": ["spmm/csr"] * 5, "stencil7": ["spmm/stencil7-row-lds"] * 5}
    try:
        for kind, names in want.items():
            assert Blab.mg3d_multi_level_product(kind) == 0
            op, m = open_operator(Blab, e, n)
            pc = Blab.Precond.multigrid3d_multi(op, nu, 0, KMAX)
            assert [pc.multigrid_level_spmm(l) for l in range(5)] == names and pc.multigrid_level_spmm(5) == "none", kind
            assert op.spmm_variant() == "spmm/csr"  # the operator's own plan is not the levels'
            R = np.random.default_rng(n).standard_normal((KMAX, n ** 3))
            alone = np.stack([apply_single(Blab, pc, op, R[j]) for j in range(KMAX)])
            for k in (1, 3, 8):
                got = apply_multi(Blab, pc, op, R[:k])
                for j in range(k):
                    assert same_bits(got[j], alone[j]), (kind, k, j, int(np.sum(got[j] != alone[j])))
            old = Blab.Precond.multigrid3d(op, nu)
            assert old.multigrid_level_spmm(0) == "none"
            old.destroy()
            pc.destroy()
            op.free()
        assert Blab.mg3d_multi_level_product("stencil7") == 0
        name, nu, tol, iterations = "poisson33", 2, 1e-6, 8
        A, en, n, Bk, X0 = batch_of(name)
        op, m = open_operator(Blab, en, n)
        pc = Blab.Precond.multigrid3d_multi(op, nu, 0, 3)
        assert pc.multigrid_level_spmm(0) == "spmm/stencil7-row-lds"
        levels = with_bounds(own_levels(name, A, n), nu, pc.multigrid_info()[2])
        X, hists, stats = Blab.pcg_solve_multi(op, m, pc, Bk, X0, tol=tol)
        for j in range(len(Bk)):
            x, hist, its, converged, breakdown = MM3.solve_levels(levels, Bk[j], X0[j], tol)
            assert stats[j].iterations == its and stats[j].converged == 1 and same_bits(hists[j], hist) and same_bits(X[j], x), (name, j)
        assert stats[0].iterations == iterations
        pc.destroy()
        op.free()
        assert Blab.mg3d_multi_level_product("smoothest") != 0 and Blab.mg3d_multi_level_product(None) != 0
    finally:
        assert Blab.mg3d_multi_level_product("auto") == 0
        Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- whole solves
@functools.lru_cache(maxsize=2)
def batch_of(name):
    """A table system with k = 3 distinct right-hand sides: the table's own (b, x0), ones from zero, a random pair."""
    A, b, x0, n = M3.table_system(name)
    N = len(b)
    rng = np.random.default_rng(N + len(name))
    Bk = np.stack([b, np.ones(N), rng.standard_normal(N)])
    X0 = np.stack([x0, np.zeros(N), rng.standard_normal(N)])
    return A, P.entries_of(A), n, Bk, X0


def open_system(B, name, nu, max_rhs=KMAX):
    A, e, n, Bk, X0 = batch_of(name)
    op, m = open_operator(B, e, n)
    return A, n, Bk, X0, op, m, B.Precond.multigrid3d_multi(op, nu, 0, max_rhs)


@pytest.mark.parametrize("name,nu,tol,iterations", ROWS)
def test_whole_solves_bit_for_bit_against_the_restatement(B, name, nu, tol, iterations):
    A, n, Bk, X0, op, m, pc = open_system(B, name, nu)
    try:
        _, grids, lmax = pc.multigrid_info()
        own = own_levels(name, A, n)
        assert max(ulps(g, L.lambda_max) for g, L in zip(lmax, own)) <= 4
        levels = with_bounds(own, nu, lmax)  # the library's reported bounds
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0, tol=tol)
        for j in range(len(Bk)):
            x, hist, its, converged, breakdown = MM3.solve_levels(levels, Bk[j], X0[j], tol)
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
    """Four columns of poisson32 that stop in three different iterations: each has the bits of the same column solved alone at k = 1 (so no
    launch after a column stopped moved a bit of its x, history or count, and no column's bits depend on k or its slot). Then b = 0
    beside two of them: p.Ap = 0 breaks it down in iteration 1 by the existing rule, its x stays zero, the others keep their bits."""
    A, n, Bk3, X03, op, m, pc = open_system(B, "poisson32", 1)
    try:
        N = n ** 3
        # from x0 = 0 the restated column takes 8 iterations on the table's b and on a random one, 7 on the alternating +-1 and 9 on
        # the ramp row / N, each with its last two residuals more than a factor 2 from the bound
        rng = np.random.default_rng(3)
        Bk = np.stack([Bk3[0], np.where(np.arange(N) % 2 == 0, 1.0, -1.0), rng.standard_normal(N), np.arange(N) / N])
        X0 = np.zeros_like(Bk)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        counts = [st.iterations for st in stats]
        assert all(st.converged == 1 for st in stats) and counts == [8, 7, 8, 9], counts
        for j in range(len(Bk)):
            x1, h1, s1 = B.pcg_solve_multi(op, m, pc, Bk[j:j + 1], X0[j:j + 1])
            assert s1[0].iterations == counts[j] and same_bits(x1[0], X[j]) and same_bits(h1[0], hists[j]), (j, counts)
        for slot in (0, 1, 2):
            mixed = np.insert(Bk[[0, 2]], slot, np.zeros(N), axis=0)
            Xm, hm, sm = B.pcg_solve_multi(op, m, pc, mixed, np.zeros((3, N)))
            assert sm[slot].converged == 0 and sm[slot].iterations == 1 and len(hm[slot]) == 2, slot
            assert np.all(Xm[slot] == 0.0)
            for at, j in zip([i for i in range(3) if i != slot], (0, 2)):
                assert same_bits(Xm[at], X[j]) and same_bits(hm[at], hists[j]) and sm[at].iterations == counts[j], (slot, j)
    finally:
        pc.destroy()
        op.free()


def test_detailed_timers_change_no_bit(B):
    A, n, Bk, X0, op, m, pc = open_system(B, "poisson33", 1, max_rhs=4)
    try:
        plain = B.pcg_solve_multi(op, m, pc, Bk, X0)
        timed = B.pcg_solve_multi(op, m, pc, Bk, X0, timers=1)
        assert same_bits(plain[0], timed[0]) and all(same_bits(a, c) for a, c in zip(plain[1], timed[1]))
        assert [s.iterations for s in plain[2]] == [s.iterations for s in timed[2]] and all(s.converged == 1 for s in timed[2])
        t = timed[2][0]
        assert t.time_spmv_ms > 0 and t.time_blas1_ms > 0 and t.time_reductions_ms > 0
        assert t.time_spmv_ms + t.time_blas1_ms + t.time_reductions_ms <= t.time_total_ms
        assert plain[2][0].time_spmv_ms == 0 and plain[2][0].time_blas1_ms == 0 and plain[2][0].time_total_ms > 0
    finally:
        pc.destroy()
        op.free()


def test_a_larger_grid_device_against_device(B):
    """64^3 Poisson at k = 2 (level 0's single path is row-lds, four levels below it): the block application against two single
    applications bit for bit, and the batched solve's iteration counts against the single solves' on the same handle. The two loops
    sum their dot products in different shapes and agree to rounding, not bit for bit; poisson64 nu 1 keeps its last two residuals 15 %
    clear of the bound on the table's column (multigrid3d_restatement.TABLE), so that column's count is the table's in both."""
    A, b, x0, n = M3.table_system("poisson64")
    N = n ** 3
    op, m = open_operator(B, P.entries_of(A), n)
    pc = B.Precond.multigrid3d_multi(op, 1, 0, 2)
    try:
        rng = np.random.default_rng(64)
        Bk, X0 = np.stack([b, rng.standard_normal(N)]), np.stack([x0, np.zeros(N)])
        got = apply_multi(B, pc, op, Bk)
        for j in range(2):
            assert same_bits(got[j], apply_single(B, pc, op, Bk[j])), j
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        for j in range(2):
            x1, h1, s1 = B.pcg_solve_device(op, m, pc, Bk[j], X0[j])
            print(f"poisson64 column {j}: batched {stats[j].iterations} iterations, single {s1.iterations}; last residuals "
                  f"{hists[j][-1] / hists[j][0]:.4e} {h1[-1] / h1[0]:.4e}")
            assert stats[j].converged == s1.converged == 1 and stats[j].iterations == s1.iterations, (j, stats[j].iterations, s1.iterations)
            assert np.max(np.abs(X[j] - x1)) <= 1e-8 * np.max(np.abs(x1)), j
        assert stats[0].iterations == 9  # the table's row
    finally:
        pc.destroy()
        op.free()


def test_the_default_level_product_on_a_large_grid(B):
    """256^3, the threshold grid: level 0's block product is spmm/stencil7-row-lds by default (128 and below: spmm/csr), level 0's single
    path stencil7/row-lds. The block application on two columns against two single applications, device against device, bit for bit."""
    n, k = 256, 2
    N = n ** 3
    op = B.Operator("stencil7-csr")
    assert op.init_synthetic3d(n, 6.0, -1.0) == 0 and op.variant() == "stencil7/row-lds" and op.spmm_variant() == "spmm/csr"
    pc = B.Precond.multigrid3d_multi(op, 1, 0, k)
    try:
        assert pc.multigrid_info()[1] == [256, 128, 64, 32, 16, 8]
        rng = np.random.default_rng(n)
        cols = rng.standard_normal((k, N))
        R, Z = B.DeviceVector.from_host(np.ascontiguousarray(cols.T).ravel()), B.DeviceVector(N * k, fill=np.nan)
        r, z = B.DeviceVector(N), B.DeviceVector(N, fill=np.nan)
        pc.apply_device_multi(op, k, R.ptr, Z.ptr)
        block = Z.to_host().reshape(N, k)
        for j in range(k):
            B.lib().spmv_amd_copy_to_device(r.ptr, cols[j].ctypes.data, cols[j].nbytes)
            pc.apply_device(op, r.ptr, z.ptr)
            single = z.to_host()
            assert same_bits(np.ascontiguousarray(block[:, j]), single), (j, int(np.sum(block[:, j] != single)))
        for v in (R, Z, r, z):
            v.free()
    finally:
        pc.destroy()
        op.free()


def test_the_handle_is_a_single_vector_handle_too(B):
    """spmv_amd_pcg_solve_device and spmv_amd_precond_apply_device with the new handle against a handle of the old 3-D creator: bit for bit."""
    A, n, Bk, X0, op, m, pc = open_system(B, "poisson33", 1, max_rhs=3)
    old = B.Precond.multigrid3d(op, 1)
    try:
        assert pc.multigrid_max_rhs() == 3 and old.multigrid_max_rhs() == 0
        (nu_a, grids_a, lmax_a), (nu_b, grids_b, lmax_b) = pc.multigrid_info(), old.multigrid_info()
        assert nu_a == nu_b and grids_a == grids_b and same_bits(lmax_a, lmax_b) and pc.multigrid_dimension() == old.multigrid_dimension() == 3
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
    n = 16  # 16^3 = 64^2 rows: the 2-D operator further down has the same size, so a handle is refused for its owner, not its size
    rows = n ** 3
    op, m = open_operator(B, S7.coo(n, center=7.0, off=-1.0), n)
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

    two = B.Precond.multigrid3d_multi(op, 1, 0, 2)
    assert two.multigrid_max_rhs() == 2 and two.multigrid_dimension() == 3
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
    for r_ptr, z_ptr in ((dR.ptr + 8, dZ.ptr), (dR.ptr, dZ.ptr + 8)):  # a block vector 8 bytes off
        with pytest.raises(RuntimeError):
            two.apply_device_multi(op, 1, r_ptr, z_ptr)
        assert "16-byte aligned" in capfd.readouterr().err
    solves(two)

    old = B.Precond.multigrid3d(op, 1)  # a handle of the old 3-D creator keeps its sentence
    refused(old, "[PCG-MULTI]", "kind 'multigrid' keeps single vectors on every level of its hierarchy", k=2)
    with pytest.raises(RuntimeError):
        old.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
    assert "single vectors" in capfd.readouterr().err
    old.destroy()
    solves(two)

    n5 = 64  # the 2-D operator beside it: each block creator refuses the other's operator, each solver the other's handle
    B.lib().spmv_amd_reset_host_matrices()
    m5 = B.HostMatrix(P.entries_of(P.stencil5(n5, center=4.0)), n5 * n5, n5 * n5, n5)
    op5 = B.Operator("stencil5-csr")
    assert op5.init(m5) == 0
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d_multi(op5, 1, 0, 4)
    assert info.value.bad_row == -1 and "is not stencil7-csr" in capfd.readouterr().err
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid_multi(op, 1, 0, 4)
    assert info.value.bad_row == -1 and "is not stencil5-csr" in capfd.readouterr().err
    flat = B.Precond.multigrid_multi(op5, 1, 0, 2)
    refused(flat, "made from another operator", k=2)  # a 2-D block handle on the 3-D operator
    with pytest.raises(RuntimeError):  # and the 3-D block handle on the 2-D operator
        B.pcg_solve_multi(op5, m5, two, np.ones((2, n5 * n5)), np.zeros((2, n5 * n5)))
    assert "made from another operator" in capfd.readouterr().err
    for handle, operator in ((two, op5), (flat, op)):
        with pytest.raises(RuntimeError):
            handle.apply_device_multi(operator, 2, dR.ptr, dZ.ptr)
        assert "made from another operator" in capfd.readouterr().err
    flat.destroy()
    op5.free()
    solves(two)

    assert op.init(m) == 0  # a stale one: made before the operator was last initialised
    refused(two, "refused", k=2)
    with pytest.raises(RuntimeError):
        two.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
    fresh = B.Precond.multigrid3d_multi(op, 1, 0, 3)
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


def test_a_zero_centre_is_refused_with_its_row_and_destroy_gives_the_block_vectors_back(B):
    n = 12
    good = S7.coo(n, center=7.0, off=-1.0)
    e = good.copy()
    at = np.nonzero((e["row"] == 777) & (e["col"] == 777))[0][0]
    e["value"][at] = 0.0
    op, m = open_operator(B, e, n)
    before = _free_bytes()
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d_multi(op, 1, 0, 8)
    assert info.value.bad_row == 777
    assert _free_bytes() >= before  # nothing of the refused hierarchy stayed on the device
    op.free()
    # destroy() gives the block vectors back: R, D, Z, W of 8 columns on every level above 0 (a grid large enough for the allocations to
    # show in the device's free bytes)
    n = 128
    assert op.init_synthetic3d(n) == 0
    pc = B.Precond.multigrid3d_multi(op, 1, 0, 8)
    held = _free_bytes()
    pc.destroy()
    assert _free_bytes() - held >= 4 * 8 * (n // 2) ** 3 * 8
    op.free()
