"""The AMG hierarchy with block vectors on the GPU (spmv_amd_precond_create_amg_multi: csrc/amg.hip, csrc/amg_multi.hip and the cycle of
csrc/multigrid_multi.hip): the handle against a handle of spmv_amd_precond_create_amg level by level; the block
application bit for bit per column against tests/pcg_multi_amg_restatement.py, whatever k and the slot, and against the single-vector
application where the levels' variants make the bits coincide; whole batched PCG and GCR(16) solves bit for bit (x, history, count),
with columns that stop in different iterations, a zero column and a NaN column; the handle as a single-vector one; the refusals that
stay; and a clean batched solve on the remains of one that ended badly."""
import numpy as np
import pytest

import amg_restatement as AMG
import csr_restatement as CSR
import gcr_restatement as GR
import leftovers as LO
import pcg_multi_amg_restatement as PA
from bitwise import same_bits

pytestmark = pytest.mark.gpu

KMAX = 8
# (name, matrix, theta): the arrow at theta = 0 has aggregates of thousands of members and hub rows of 2 500 entries
SYSTEMS = {"poisson33": (lambda: AMG.system("poisson33")[0], AMG.THETA), "nine24": (lambda: AMG.system("nine24")[0], AMG.THETA),
           "cube9": (lambda: AMG.system("cube9")[0], AMG.THETA), "graph1500": (lambda: AMG.system("graph1500")[0], AMG.THETA),
           "arrow-theta0": (AMG.arrow, 0.0)}


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def open_csr(Bx, M):
    """cusparse-csr holding M, in the automatic variant."""
    Bx.lib().spmv_amd_reset_host_matrices()
    rows = AMG.rows_of(M)
    m = Bx.HostMatrix(CSR.entries_of(M.rp, M.ci, M.va), rows, rows, -1)
    op = Bx.Operator("cusparse-csr")
    op.select_variant(None)
    assert op.init(m) == 0
    return op, m


def apply_multi(B, pc, op, cols):
    """The block application on the columns `cols` (k, rows); R must keep its bits. Returns (k, rows)."""
    k, rows = cols.shape
    block = np.ascontiguousarray(cols.T).ravel()
    dR, dZ = B.DeviceVector.from_host(block), B.DeviceVector(rows * k, fill=np.nan)
    pc.apply_device_multi(op, k, dR.ptr, dZ.ptr)
    got = dZ.to_host().reshape(rows, k)
    assert same_bits(dR.to_host(), block), "R changed"
    dR.free(), dZ.free()
    return np.ascontiguousarray(got.T)


def apply_single(B, pc, op, r):
    dr, dz = B.DeviceVector.from_host(np.ascontiguousarray(r)), B.DeviceVector(len(r), fill=np.nan)
    pc.apply_device(op, dr.ptr, dz.ptr)
    z = dz.to_host()
    dr.free(), dz.free()
    return z


# ---------------------------------------------------------------- the handle
@pytest.mark.parametrize("name", ["poisson33", "graph1500", "arrow-theta0"])
def test_the_hierarchy_is_the_single_creators(Blab, name):
    """amg_info and every level's map, CSR, dinv and lambda_max equal those of a Precond.amg handle on the same operator bit for bit;
    max_rhs is reported; destroy, then create again."""
    make, theta = SYSTEMS[name]
    op, _ = open_csr(Blab, make())
    try:
        old = Blab.Precond.amg(op, 1, 0, theta)
        new = Blab.Precond.amg_multi(op, 1, 0, theta, 3)
        assert (new.multigrid_max_rhs(), old.multigrid_max_rhs()) == (3, 0)
        assert new.kind == "multigrid" and new.multigrid_dimension() == 0 and new.chebyshev_info() is None
        a, b = new.amg_info(), old.amg_info()
        assert a["setup_ms"] > 0.0
        for key in ("smoother_degree", "strength", "rows", "nnz", "max_aggregate"):
            assert a[key] == b[key], (name, key)
        assert same_bits(a["lambda_max"], b["lambda_max"]) and len(a["rows"]) >= 2
        (nu_a, grids_a, lmax_a), (nu_b, grids_b, lmax_b) = new.multigrid_info(), old.multigrid_info()
        assert nu_a == nu_b == 1 and grids_a == grids_b == [0] * len(a["rows"]) and same_bits(lmax_a, lmax_b)
        for l in range(len(a["rows"])):
            for got, want in zip(new.amg_level(l), old.amg_level(l)):
                assert (got is None) == (want is None), (name, l)
                if got is not None:
                    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, l)
            assert new.multigrid_level_spmm(l) == "spmm/csr" and old.multigrid_level_spmm(l) == "none", (name, l)
        assert same_bits(new.inverse_diagonal(), old.inverse_diagonal())
        new.destroy()
        again = Blab.Precond.amg_multi(op, 1, 0, theta, KMAX)  # lifetime: destroy, then create again
        assert again.multigrid_max_rhs() == KMAX and again.amg_info()["rows"] == b["rows"]
        again.destroy(), old.destroy()
    finally:
        op.free()


# ---------------------------------------------------------------- the block application, bit for bit
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_application_bit_for_bit(B, name):
    """Per column the restatement's bits at k = 1, 3 and 8 (so they depend neither on k nor on the other columns) and in another slot
    (the columns permuted). Where every level's single-vector product runs csr/stream or csr/row-scalar -- every system here but the
    arrow -- spmv_amd_precond_apply_device gives the same bits on this handle and on a Precond.amg handle. On the arrow level 0 runs
    csr/adaptive: its hub rows are summed as a tree by the single path and as the sequential chain by the block path, two roundings
    of one cycle; they are held to a relative 1e-12, a rounding-level bound (2 500 terms of unit roundoff 1.1e-16 under a cycle whose
    operator norm is O(1)), not a tolerance fitted to the result."""
    make, theta = SYSTEMS[name]
    M = make()
    rows = AMG.rows_of(M)
    op, _ = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, 1, 0, theta, KMAX)
        levels = AMG.hierarchy(M, 1, 0, theta)
        assert pc.amg_info()["rows"] == [L.rows for L in levels], name
        coincide = PA.bits_coincide(levels)
        assert coincide == (name != "arrow-theta0") and (coincide or op.variant() == "csr/adaptive"), (name, PA.level_variants(levels))
        if not coincide:
            assert int(np.diff(levels[0].g.agg_ptr).max()) > 1000 and int(np.diff(M.rp).max()) >= 2500
        R = np.random.default_rng(rows + 26).standard_normal((KMAX, rows))
        cycle = PA.make_cycle(levels)
        want = np.stack([cycle(R[j]) for j in range(KMAX)])
        for k in (1, 3, 8):
            got = apply_multi(B, pc, op, R[:k])
            for j in range(k):
                assert same_bits(got[j], want[j]), (name, k, j, int(np.sum(got[j] != want[j])), float(np.max(np.abs(got[j] - want[j]))))
        perm = [3, 4, 5, 6, 7, 0, 1, 2]
        moved = apply_multi(B, pc, op, R[perm])
        for slot, j in enumerate(perm):
            assert same_bits(moved[slot], want[j]), (name, "slot", slot, j)
        old = B.Precond.amg(op, 1, 0, theta)
        for j in (0, 5):
            for handle in (pc, old):
                single = apply_single(B, handle, op, R[j])
                if coincide:
                    assert same_bits(single, want[j]), (name, j, handle is pc)
                else:
                    assert np.linalg.norm(single - want[j]) <= 1e-12 * np.linalg.norm(single), (name, j)
        old.destroy(), pc.destroy()
    finally:
        op.free()


def test_capacity_and_the_refusals_that_stay(B, capfd):
    """nrhs > max_rhs is refused by the existing sentence; batched BiCGSTAB refuses the handle; a Precond.amg handle is still refused by
    the three batched entry points with today's sentence; the operator re-initialised under a live handle is refused by generation."""
    M, _ = AMG.system("poisson33")
    rows = AMG.rows_of(M)
    op, m = open_csr(B, M)
    Bk, X0 = np.ones((3, rows)), np.zeros((3, rows))
    dR, dZ = B.DeviceVector.from_host(np.ones(3 * rows)), B.DeviceVector(3 * rows, fill=0.0)
    try:
        two = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 2)
        for call in (lambda: B.pcg_solve_multi(op, m, two, Bk, X0), lambda: B.gcr_solve_multi(op, m, two, Bk, X0, restart=4),
                     lambda: two.apply_device_multi(op, 3, dR.ptr, dZ.ptr)):
            capfd.readouterr()
            with pytest.raises(RuntimeError):
                call()
            err = capfd.readouterr().err
            assert "nrhs = 3" in err and "max_rhs = 2" in err, err
        X, _, stats = B.pcg_solve_multi(op, m, two, Bk[:2], X0[:2])
        assert all(s.converged == 1 for s in stats)
        capfd.readouterr()
        with pytest.raises(RuntimeError):  # BiCGSTAB keeps refusing the kind
            B.bicgstab_solve_multi(op, m, two, Bk[:2], X0[:2])
        assert "multigrid" in capfd.readouterr().err
        old = B.Precond.amg(op, 1)
        for batched in (lambda: B.pcg_solve_multi(op, m, old, Bk[:2], X0[:2]), lambda: B.gcr_solve_multi(op, m, old, Bk[:2], X0[:2]),
                        lambda: old.apply_device_multi(op, 2, dR.ptr, dZ.ptr)):
            capfd.readouterr()
            with pytest.raises(RuntimeError):
                batched()
            assert "keeps single vectors on every level" in capfd.readouterr().err
        old.destroy()
        assert op.init(m) == 0  # a stale handle: made before the operator was last initialised
        with pytest.raises(RuntimeError):
            B.pcg_solve_multi(op, m, two, Bk[:2], X0[:2])
        with pytest.raises(RuntimeError):
            two.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
        with pytest.raises(RuntimeError):
            B.pcg_solve_device(op, m, two, Bk[0], X0[0])
        two.destroy()
        fresh = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 2)
        _, _, stats = B.pcg_solve_multi(op, m, fresh, Bk[:2], X0[:2])
        assert all(s.converged == 1 for s in stats)
        fresh.destroy()
    finally:
        dR.free(), dZ.free()
        op.free()


# ---------------------------------------------------------------- whole solves
def four_columns(name):
    """The table's b, ones, the alternating +-1 and the ramp row / N, all from x0 = 0: the restated columns stop in different
    iterations (poisson33: 12, 13, 9, 13; graph1500: 18, 19, 19, 19), so a column is frozen while the others run on."""
    n = AMG.rows_of(AMG.system(name)[0])
    return np.stack([AMG.vectors(name)[0], np.ones(n), np.where(np.arange(n) % 2 == 0, 1.0, -1.0), np.arange(n) / n]), np.zeros((4, n))


@pytest.mark.parametrize("name", ["poisson33", "graph1500"])
def test_pcg_solve_multi_bit_for_bit(B, name):
    """k = 4: x, the history and the count of every column against the restatement; the same solve twice gives the same bits."""
    M, st = AMG.system(name)
    Bk, X0 = four_columns(name)
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 4)
        levels = AMG.hierarchy(M, 1, levels=st)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        counts = []
        for j in range(4):
            x, hist, its, converged, breakdown = PA.solve_levels(levels, Bk[j], X0[j])
            counts.append(its)
            assert converged and not breakdown and stats[j].iterations == its and stats[j].converged == 1, (name, j, stats[j].iterations, its)
            assert same_bits(hists[j], hist), (name, j, [float(v) for v in hists[j][:3]], [float(v) for v in hist[:3]])
            assert same_bits(X[j], x), (name, j, int(np.sum(X[j] != x)))
        assert min(counts) < max(counts) and counts[0] == {(n, nu): its for n, nu, its in AMG.TABLE}[(name, 1)], counts
        again = B.pcg_solve_multi(op, m, pc, Bk, X0)
        assert same_bits(again[0], X) and all(same_bits(a, c) for a, c in zip(again[1], hists))
        pc.destroy()
    finally:
        op.free()


def test_a_zero_column_and_a_nan_column_beside_healthy_ones(B):
    """b = 0 in slot 1 and a NaN in b in slot 2: both break down in iteration 1 by the existing rule and their x stays x0 = 0; the healthy
    columns in slots 0 and 3 keep the restatement's bits -- nothing of the NaN column reaches them through any level of the cycle."""
    M, st = AMG.system("poisson33")
    Bk, X0 = four_columns("poisson33")
    Bk[1] = 0.0
    Bk[2] = Bk[0]
    Bk[2, 17] = np.nan
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 4)
        levels = AMG.hierarchy(M, 1, levels=st)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        for j in (1, 2):
            assert stats[j].converged == 0 and stats[j].iterations == 1 and len(hists[j]) == 2 and np.all(X[j] == 0.0), (j, stats[j].iterations)
        assert np.all(hists[1] == 0.0) and np.all(np.isnan(hists[2]))
        for j in (0, 3):
            x, hist, its, converged, _ = PA.solve_levels(levels, Bk[j], X0[j])
            assert converged and stats[j].iterations == its and stats[j].converged == 1, (j, stats[j].iterations, its)
            assert same_bits(hists[j], hist) and same_bits(X[j], x), j
        pc.destroy()
    finally:
        op.free()


def test_gcr_solve_multi_on_the_upwind_stencil_bit_for_bit(B):
    """GCR(16) at k = 3 on the 33 x 33 upwind stencil against gcr_multi_restatement's loop with the cycle as the application; the
    table's own column takes the table's count."""
    name, nu, restart, iterations = AMG.GCR_ROW
    M, b, x0 = AMG.upwind33()
    n = len(b)
    Bk = np.stack([b, np.ones(n), np.random.default_rng(n + 3).standard_normal(n)])
    X0 = np.stack([x0, np.zeros(n), np.zeros(n)])
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, nu, 0, AMG.THETA, 3)
        levels = AMG.hierarchy(M, nu)
        assert pc.amg_info()["rows"] == [L.rows for L in levels]
        X, hists, stats = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart)
        for j in range(3):
            x, hist, its, converged, end = PA.gcr_levels(levels, Bk[j], X0[j], restart)
            assert converged and end == "converged" and stats[j].iterations == its and stats[j].converged == 1, (j, stats[j].iterations, its)
            assert same_bits(hists[j], hist) and same_bits(X[j], x), (j, int(np.sum(X[j] != x)))
        assert stats[0].iterations == iterations
        pc.destroy()
    finally:
        op.free()


def test_the_handle_is_a_single_vector_handle_too(B, O):
    """spmv_amd_pcg_solve_device and spmv_amd_gcr_solve_device on the new handle against amg_restatement.pcg_exact and
    gcr_restatement.gcr_exact, as tests/test_amg_gpu.py holds a Precond.amg handle to them."""
    M, st = AMG.system("poisson33")
    b, x0 = AMG.vectors("poisson33")
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 2)
        levels = AMG.hierarchy(M, 1, levels=st)
        xo, ho, ito, conv = AMG.pcg_exact(O, M, AMG.exact_cycle(O, levels, op.variant()), b, x0, variant0=op.variant())
        x, h, stats = B.pcg_solve_device(op, m, pc, b, x0)
        assert conv and stats.converged == 1 and stats.iterations == ito == 12, (stats.iterations, ito)
        assert same_bits(h, ho) and same_bits(x, xo)
        pc.destroy()
    finally:
        op.free()
    name, nu, restart, iterations = AMG.GCR_ROW
    M, b, x0 = AMG.upwind33()
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg_multi(op, nu, 0, AMG.THETA, 2)
        levels = AMG.hierarchy(M, nu)
        want = GR.gcr_exact(lambda v: O.spmv_csr(M.rp, M.ci, M.va, v), b, x0, AMG.exact_cycle(O, levels, op.variant()), restart)
        x, h, stats = B.gcr_solve(op, m, pc, b, x0, restart=restart)
        assert stats.converged == 1 and stats.iterations == want[2] == iterations, (stats.iterations, want[2])
        assert same_bits(h, want[1]) and same_bits(x, want[0])
        pc.destroy()
    finally:
        op.free()


# ---------------------------------------------------------------- a clean batched solve on the remains of one that ended badly
@pytest.mark.parametrize("clean", LO.CLEAN, ids=[c.name for c in LO.CLEAN])
def test_a_batched_solve_inherits_nothing_from_the_one_before(B, clean):
    """The rows of tests/leftovers.py on the 33 x 33 Poisson matrix in cusparse-csr, two columns per solve: behind every dirtying
    batched solve -- NaN and inf right-hand sides, a zero one, no iterations, huge junk, an early stop --, on the same workspace, the
    same handle and the same level vectors, the clean batched solve gives the bits it gave on a fresh workspace and a fresh handle."""
    grid, k = 33, 2
    M, _ = AMG.system("poisson33")
    op, m = open_csr(B, M)
    handle = {}

    def solve(d):
        if "pc" not in handle:
            handle["pc"] = B.Precond.amg_multi(op, 1, 0, AMG.THETA, k)
        pairs = [LO.vectors(d, grid, 2, seed=j) for j in range(k)]
        X, hists, stats = B.pcg_solve_multi(op, m, handle["pc"], np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]),
                                            max_iters=d.max_iters, tol=d.tol)
        return [LO.column_of(X[j], hists[j], stats[j]) for j in range(k)]

    solve.last_history = lambda j, buf: B._pcg_lib().spmv_amd_pcg_last_history_multi(j, buf.ctypes.data, len(buf))

    def release():
        B.lib().spmv_amd_cg_release_workspace()
        if "pc" in handle:
            handle.pop("pc").destroy()

    try:
        fresh = LO.dirty_then_clean(solve, release, clean, LO.DIRTY)
        for f in fresh:
            assert np.all(np.isfinite(f.x)) and len(f.history) == f.iterations + 1
            if clean.name.startswith("converging"):
                assert f.converged == 1
    finally:
        release()
        op.free()
