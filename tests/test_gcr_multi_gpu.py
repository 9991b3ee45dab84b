"""Batched GCR(m) on the GPU (spmv_amd_gcr_solve_device_multi, csrc/gcr_multi.hip), through the product library: every column of
every solve BIT for bit (x, history, count, converged) against the numpy restatement on that operator's own product
(tests/gcr_multi_restatement.py), the application of kinds "chebyshev" and "multigrid" handed in through the library's own
spmv_amd_precond_apply_device_multi -- whole solves on stencil5-csr, cusparse-csr and stencil7-csr under all four kinds, both block
hierarchies included, at k = 1, 3 and 8 and restart 1, 4 and 16, whose columns stop in different iterations and so exercise freezing;
column independence; a poisoned and a zero neighbour; every end of the loop in one batch; the two-stage sum; determinism; agreement
with the single-RHS solver; the workspace; the refusals that need a device. The inputs are shown to be sound by
tests/test_gcr_multi_host.py, the kernels one by one by tests/test_gcr_multi_stages_gpu.py."""
import ctypes as C
import re

import numpy as np
import pytest

import gcr_multi_restatement as GM
import gcr_restatement as GR
from bitwise import same_bits
from gcr_restatement import entries_of, hist_err, table_system, third_rounding_bound
from test_gcr_multi_host import ENDS, ENDS_B, ENDS_CAP, ENDS_ITERATIONS, ENDS_RESTART, ENDS_TOL, ends_entries

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
# (system, operator, kind, restart): every row of the restatement's table on the stencil operator of its dimension, and two of them on
# cusparse-csr (another product, so other bits; the counts hold)
SOLVES = [(c[0], "stencil7-csr" if c[0].startswith("cube") else "stencil5-csr", c[1], c[2]) for c in GM.CASES]
SOLVES += [("grid33", "cusparse-csr", "none", 4), ("grid33", "cusparse-csr", "jacobi", 16)]


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_reset_host_matrices()


def open_operator(B, name, mode):
    A, _, _ = table_system(name)
    m = B.HostMatrix(entries_of(A), A.shape[0], A.shape[0], GR.grid_of(A, GR.dimension_of(name)))
    op = B.Operator(mode)
    assert op.init(m) == 0
    return op, m


def make_precond(B, op, kind, dim, max_rhs=8):
    name, nu = GR.parse_kind(kind)
    if name == "chebyshev":
        return B.Precond.chebyshev(op, nu)
    if name == "multigrid":
        return B.Precond.multigrid_multi(op, nu, max_rhs=max_rhs) if dim == 2 else B.Precond.multigrid3d_multi(op, nu, max_rhs=max_rhs)
    return B.Precond(op, name)


class BlockApply:
    """r -> z = M^-1 r of ONE column through spmv_amd_precond_apply_device_multi (k = 1: a column's bits do not depend on k)."""

    def __init__(self, B, op, pc, n):
        self.B, self.op, self.pc = B, op, pc
        self.r, self.z = B.DeviceVector(n, 0.0), B.DeviceVector(n, 0.0)

    def __call__(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        self.B.lib().spmv_amd_copy_to_device(self.r.ptr, r.ctypes.data, r.nbytes)
        self.pc.apply_device_multi(self.op, 1, self.r.ptr, self.z.ptr)
        return self.z.to_host()

    def free(self):
        self.r.free(), self.z.free()


_products, _restated = {}, {}


def product_of(O, name, mode):
    """The operator's own product: oracle.spmv_stencil5 for stencil5-csr, oracle.spmv_csr for the others."""
    key = (name, mode == "stencil5-csr")
    if key not in _products:
        A, _, _ = table_system(name)
        rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
        grid = GR.grid_of(A, GR.dimension_of(name))
        _products[key] = (lambda u: O.spmv_stencil5(rp, ci, va, u, grid)) if key[1] else (lambda u: O.spmv_csr(rp, ci, va, u))
    return _products[key]


def restated(B, O, op, pc, name, mode, kind, restart, seed, tol=GM.TOL, max_iters=1000):
    """The restatement of column `seed` of the system (0: the table system; 1..8: the seeded columns) on the operator's product:
    computed once, shared by every test that needs it."""
    key = (name, mode == "stencil5-csr", kind, restart, seed, tol, max_iters)
    if key not in _restated:
        A, _, _ = table_system(name)
        b, x0 = GM.column(name, seed)
        base, _ = GR.parse_kind(kind)
        owned = None
        if base == "none":
            apply = lambda r: r
        elif base == "jacobi":
            dinv = 1.0 / GR.diagonal(A)
            apply = lambda r: dinv * r
        else:
            apply = owned = BlockApply(B, op, pc, A.shape[0])
        try:
            _restated[key] = GM.solve(product_of(O, name, mode), b, x0, apply, restart, tol, max_iters)
        finally:
            if owned is not None:
                owned.free()
    return _restated[key]


def check_column(got, j, want, label):
    """Column j of (X, hists, stats) against (x, history, iterations, converged, end) of the restatement, bit for bit."""
    X, hists, stats = got
    x, hist, its, converged, _ = want
    assert (stats[j].iterations, stats[j].converged) == (its, int(converged)), (label, j, stats[j].iterations, stats[j].converged, its)
    assert len(hists[j]) == len(hist), (label, j)
    diff = np.flatnonzero(np.ascontiguousarray(hists[j]).view(np.uint64) != np.ascontiguousarray(hist).view(np.uint64))
    assert len(diff) == 0, (label, j, "history differs first at", int(diff[0]), float(hists[j][diff[0]]), float(hist[diff[0]]))
    assert same_bits(X[j], x), (label, j, int(np.sum(X[j] != x)))


def stats_tuple(s):
    return (s.iterations, s.converged, s.residual_norm, s.solution_sum, s.solution_norm)


def batch_of(name, seeds):
    cols = [GM.column(name, s) for s in seeds]
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols])


# ---------------------------------------------------------------- whole solves, bit for bit
@pytest.mark.parametrize("name, mode, kind, restart", SOLVES, ids=[f"{s[0]}-{s[1]}-{s[2]}-m{s[3]}" for s in SOLVES])
def test_whole_solves_bit_for_bit_against_the_restatement(B, O, name, mode, kind, restart):
    """Columns 0 .. k - 1 of the table at k = 1, 3 and 8 (the 8-byte and the 16-byte walk): each takes the table's count and ending and
    equals its restatement in x, history, count and verdict. The columns of a batch stop in different iterations, so all but the last
    spend iterations frozen beside running ones; restart 16 passes both chunk boundaries and wraps, restart 1 restarts every iteration."""
    op, m = open_operator(B, name, mode)
    pc = make_precond(B, op, kind, GR.dimension_of(name))
    try:
        for k in KS:
            Bk, X0 = batch_of(name, range(k))
            got = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart)
            for j in range(k):
                want = restated(B, O, op, pc, name, mode, kind, restart, j)
                iterations, end, _ = GM.TABLE[(name, kind, restart, j)]
                assert (want[2], want[4]) == (iterations, end) and want[3], (name, kind, restart, j, want[2:])
                check_column(got, j, want, (name, mode, kind, restart, k))
                assert got[2][j].residual_norm == got[1][j][-1]
        assert len({s.iterations for s in got[2]}) >= 2  # k = 8: the columns stop in different iterations
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- independence, bad neighbours
@pytest.mark.parametrize("kind, restart", [("none", 16), ("multigrid1", 4)])
def test_a_column_has_the_same_bits_in_every_batch(B, O, kind, restart):
    """Seeded column 4 of grid65 alone, in slot 0 of three and in slot 7 of eight: the same x, history and statistics."""
    name, mode = "grid65", "stencil5-csr"
    op, m = open_operator(B, name, mode)
    pc = make_precond(B, op, kind, 2)
    try:
        alone = B.gcr_solve_multi(op, m, pc, *batch_of(name, [4]), restart=restart)
        check_column(alone, 0, restated(B, O, op, pc, name, mode, kind, restart, 4), "k = 1")
        for ids, slot in (([4, 0, 7], 0), ([0, 1, 2, 3, 5, 6, 7, 4], 7)):
            got = B.gcr_solve_multi(op, m, pc, *batch_of(name, ids), restart=restart)
            assert same_bits(got[0][slot], alone[0][0]) and same_bits(got[1][slot], alone[1][0]), (len(ids), slot)
            assert stats_tuple(got[2][slot]) == stats_tuple(alone[2][0])
            for s, j in enumerate(ids):
                check_column(got, s, restated(B, O, op, pc, name, mode, kind, restart, j), (ids, s))
    finally:
        pc.destroy()
        op.free()


@pytest.mark.parametrize("kind, restart", [("none", 4), ("jacobi", 16), ("chebyshev2", 4), ("multigrid1", 16)])
def test_a_poisoned_and_a_zero_neighbour(B, O, kind, restart):
    """A column whose b holds an inf: ||r0|| = inf, z and q hold NaN, gamma is not finite -- breakdown in iteration 1, history [inf, inf],
    x = x0. A column with b = x0 = 0: gamma = 0, breakdown in iteration 1 with history [0, 0]. In slot 0, slot 1 and the last slot of
    k = 2 and 8 they leave every other column's bits as they are -- through the block V-cycle and the Chebyshev steps too."""
    name, mode = "grid33", "stencil5-csr"
    op, m = open_operator(B, name, mode)
    pc = make_precond(B, op, kind, 2)
    try:
        rows = 33 * 33
        healthy_b, healthy_x0 = batch_of(name, range(7))
        poisoned = np.random.default_rng(5).standard_normal(rows)
        poisoned[rows // 2 + 1] = np.inf
        for what, bad, hist in (("inf", poisoned, [np.inf, np.inf]), ("zero", np.zeros(rows), [0.0, 0.0])):
            for k in (2, 8):
                for slot in sorted({0, 1, k - 1}):
                    Bk = np.insert(healthy_b[:k - 1], slot, bad, axis=0)
                    X0 = np.insert(healthy_x0[:k - 1], slot, np.zeros(rows), axis=0)
                    got = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart)
                    X, hists, stats = got
                    label = (what, k, slot)
                    assert stats[slot].iterations == 1 and stats[slot].converged == 0 and same_bits(hists[slot], hist), (label, hists[slot])
                    assert same_bits(X[slot], np.zeros(rows)), label
                    for j, s in enumerate([s for s in range(k) if s != slot]):
                        check_column(got, s, restated(B, O, op, pc, name, mode, kind, restart, j), label)
    finally:
        pc.destroy()
        op.free()


def test_every_end_in_one_batch(B, O, capfd):
    """The 10 x 10 block-diagonal matrix of tests/test_gcr_multi_host.py, one column supported on each block, restart 1: a gamma
    breakdown, a rho breakdown, converged in iteration 1, converged in iteration 12 and the cap of 16 in ONE batch. Each column bit for
    bit -- so a column that stopped early holds, 15 iterations later, exactly the x and history it had at its freeze --, each breakdown
    line naming its scalar."""
    e = np.zeros(len(ends_entries()), dtype=B.ENTRY_DTYPE)
    for i, v in enumerate(ends_entries()):
        e[i] = v
    m = B.HostMatrix(e, 10, 10, -1)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    try:
        rp, ci, va = O.build_csr(e, 10)
        capfd.readouterr()
        got = B.gcr_solve_multi(op, m, pc, ENDS_B, np.zeros((5, 10)), restart=ENDS_RESTART, tol=ENDS_TOL, max_iters=ENDS_CAP, verbose=1)
        out = capfd.readouterr().out
        scalar = {"gamma": "gamma = q.q", "rho": "rho = r.q"}
        lines = [l for l in out.splitlines() if "Breakdown" in l]
        assert lines == [f"[GCR-MULTI {j}] Breakdown in iteration 1 ({scalar[end]} zero or not finite)" for j, end in enumerate(ENDS) if end in scalar], out
        assert "[GCR-MULTI 1] Initial residual: 1.000000e+00 (preconditioner none)" in out and "[PCG" not in out and "[GCR-DEVICE]" not in out
        for j, (end, its) in enumerate(zip(ENDS, ENDS_ITERATIONS)):
            want = GM.solve(lambda u: O.spmv_csr(rp, ci, va, u), ENDS_B[j], np.zeros(10), lambda r: r, ENDS_RESTART, ENDS_TOL, ENDS_CAP)
            assert (want[4], want[2]) == (end, its), (j, want[2:])
            check_column(got, j, want, j)
            assert got[2][j].converged == int(end == "converged")
        assert same_bits(got[0][0], np.zeros(10)) and same_bits(got[0][1], np.zeros(10))
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- the two-stage sum
def test_the_two_stage_sum_on_a_1025_grid(B, O):
    """1025^2 rows are 4 105 partials per value: a full slice of 4 096 and a second of 9, so every reducing launch publishes two slice
    sums per value and column and the last ticket sums them. One capped solve, k = 2, restart 4, 6 iterations (a restart and up to
    three betas), on the synthetic stencil (centre 5, off -1): both columns bit for bit."""
    n, cap = 1025, 6
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    pc = B.Precond(op, "jacobi")
    try:
        assert (rows + 255) // 256 == 4105
        rng = np.random.default_rng(n)
        Bk, X0 = rng.standard_normal((2, rows)), rng.standard_normal((2, rows))
        got = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=4, max_iters=cap)
        rp, ci, va = O.stencil5_csr(n)
        dinv = np.full(rows, 1.0 / 5.0)
        for j in range(2):
            want = GM.solve(lambda u: O.spmv_stencil5(rp, ci, va, u, n), Bk[j], X0[j], lambda r: dinv * r, 4, GM.TOL, cap)
            assert want[2] == cap and not want[3]
            check_column(got, j, want, j)
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- parameters, the single solver
def test_solve_parameters_and_the_single_rhs_solver(B, O, capfd):
    """A solve run twice is bit-identical, with the detailed timers too and after a solve of another kind and restart in between;
    max_iters = 0 returns x0 and one history entry; a capped solve's history is the full one's beginning; verbose changes no bit and
    tags its lines; under "none" and "jacobi" every column takes the single-RHS solver's count and ending and agrees with its history
    within the table row's margin; the single solver's history is left alone."""
    name, mode, k = "grid33", "stencil5-csr", 3
    op, m = open_operator(B, name, mode)
    pcs = {"none": B.Precond(op, "none"), "jacobi": B.Precond(op, "jacobi")}
    try:
        Bk, X0 = batch_of(name, range(k))
        for kind, restart in (("none", 4), ("jacobi", 16)):
            pc = pcs[kind]
            first = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart)
            B.gcr_solve_multi(op, m, pcs["none" if kind == "jacobi" else "jacobi"], Bk[:2], X0[:2], restart=7, max_iters=9)
            again = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart)
            timed = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart, timers=1)
            for other in (again, timed):
                assert same_bits(other[0], first[0]) and all(same_bits(a, c) for a, c in zip(other[1], first[1]))
                assert [stats_tuple(s) for s in other[2]] == [stats_tuple(s) for s in first[2]]
            st, stt = first[2][0], timed[2][0]
            assert st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0
            assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0
            assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms
            for j in range(k):  # the single-RHS solver: the same count and ending, another rounding of the sums
                x, h, s = B.gcr_solve(op, m, pc, Bk[j], X0[j], restart=restart)
                iterations, end, stored = GM.TABLE[(name, kind, restart, j)]
                bound = third_rounding_bound(stored)
                assert first[2][j].iterations == s.iterations == iterations and first[2][j].converged == s.converged == int(end == "converged"), j
                err = hist_err(first[1][j], h)
                print(f"{kind} m = {restart} column {j}: batched against single-RHS {err:.2e} (bound {bound:.0e})")
                assert err <= bound and np.max(np.abs(first[0][j] - x)) <= bound * np.max(np.abs(x)), (kind, j, err)
            L = B._gcr_multi_lib()
            hs = np.zeros(len(h) + 1)
            assert L.spmv_amd_gcr_last_history(hs.ctypes.data, len(hs)) == len(h) and same_bits(hs[:-1], h)
        kind, restart, pc = "jacobi", 16, pcs["jacobi"]
        Xz, hz, sz = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart, max_iters=0)
        X5, h5, s5 = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart, max_iters=5)
        for j in range(k):
            assert sz[j].iterations == 0 and sz[j].converged == 0 and same_bits(Xz[j], X0[j]) and same_bits(hz[j], first[1][j][:1])
            assert s5[j].iterations == 5 and s5[j].converged == 0 and same_bits(h5[j], first[1][j][:6]) and s5[j].residual_norm == h5[j][0]
            check_column((X5, h5, s5), j, restated(B, O, op, pc, name, mode, kind, restart, j, max_iters=5), ("cap", j))
        few = np.full(5, -1.0)
        assert L.spmv_amd_gcr_last_history_multi(0, few.ctypes.data, 3) == 6 and same_bits(few[:3], h5[0][:3]) and few[3] == -1.0
        assert L.spmv_amd_gcr_last_history_multi(k, few.ctypes.data, 3) == -1
        capfd.readouterr()
        loud = B.gcr_solve_multi(op, m, pc, Bk, X0, restart=restart, max_iters=5, verbose=2)
        out = capfd.readouterr().out
        assert same_bits(loud[0], X5) and all(same_bits(a, c) for a, c in zip(loud[1], h5))
        assert len(re.findall(r"\[GCR-MULTI \d\] Iter +\d+: residual", out)) == 5 * k
        assert out.count("Initial residual") == k and "(preconditioner jacobi)" in out and "[PCG" not in out and "[GCR-DEVICE]" not in out
        assert "[GCR-MULTI] 3 systems, time breakdown (whole batch):" in out and "Breakdown" not in out
        assert [s.residual_norm for s in loud[2]] == [h[5] for h in h5]
    finally:
        for p in pcs.values():
            p.destroy()
        op.free()


# ---------------------------------------------------------------- workspace
def _free_bytes():
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_workspace_goes_with_the_other_cg_workspaces(B):
    """600^2 rows at k = 2 (block vectors of 5.8 MB: large enough to show in the device's free bytes). A release -- by either release
    entry point -- gives back at least what spmv_amd_gcr_multi_workspace_bytes promised for the k, restart and kind of the solve; the
    next solve makes it again (the same bits); an operator's free() releases it too."""
    n, k = 600, 2
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    Bk = np.random.default_rng(n).standard_normal((k, rows))
    releases = (B.lib().spmv_amd_cg_release_workspace, B._pcg_lib().spmv_amd_pcg_release_workspace, B.lib().spmv_amd_cg_release_workspace)
    for (kind, restart), release in zip((("none", 4), ("jacobi", 16), ("chebyshev", 2)), releases):
        pc = B.Precond.chebyshev(op, 2) if kind == "chebyshev" else B.Precond(op, kind)
        promised = B.gcr_multi_workspace_bytes(rows, k, restart, kind)
        assert promised >= (4 + 2 * restart) * rows * k * 8
        release()
        first = B.gcr_solve_multi(op, m, pc, Bk, np.zeros((k, rows)), restart=restart, max_iters=3)
        held = _free_bytes()
        release()
        given = _free_bytes() - held
        # at least what was promised; the allocator's granularity, the slices, records and histories come on top
        assert promised <= given < 2 * promised + (64 << 20), (kind, restart, promised, given)
        again = B.gcr_solve_multi(op, m, pc, Bk, np.zeros((k, rows)), restart=restart, max_iters=3)
        assert same_bits(again[0], first[0]) and all(same_bits(a, c) for a, c in zip(again[1], first[1])) and again[2][0].iterations == 3
        pc.destroy()
    held = _free_bytes()
    op.free()
    after = _free_bytes()
    assert after - held >= B.gcr_multi_workspace_bytes(rows, k, 2, "chebyshev")
    B._pcg_lib().spmv_amd_pcg_release_workspace()
    assert _free_bytes() - after < rows * 8


# ---------------------------------------------------------------- refusals that need a device
def test_refusals_that_need_a_device(B, capfd):
    name = "grid33"
    rows = 33 * 33
    op, m = open_operator(B, name, "stencil5-csr")
    Bk, X0 = batch_of(name, range(3))

    def refused(handle, word, operator=None, matrix=None, k=3):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            B.gcr_solve_multi(operator or op, matrix or m, handle, Bk[:k], X0[:k], restart=4)
        err = capfd.readouterr().err
        assert "[GCR-MULTI]" in err and word in err, err

    single = B.Precond.multigrid(op)
    refused(single, "kind 'multigrid' keeps single vectors on every level of its hierarchy: not available for several right-hand sides, refused")
    single.destroy()
    two = B.Precond.multigrid_multi(op, max_rhs=2)
    refused(two, "nrhs = 3, the multigrid preconditioner's hierarchy holds block vectors of max_rhs = 2 columns: refused")
    X, hists, stats = B.gcr_solve_multi(op, m, two, Bk[:2], X0[:2], restart=4)  # within its capacity it solves
    assert all(s.converged == 1 for s in stats)
    two.destroy()
    jac = B.Precond(op, "jacobi")
    other = B.Operator("cusparse-csr")
    assert other.init(m) == 0
    refused(jac, "refused", operator=other)  # a handle of another operator
    small = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows - 1, rows - 1, -1)
    refused(jac, "square system of that size", matrix=small)
    short = B.Precond.from_diagonal(np.ones(rows - 1))
    refused(short, "the preconditioner is for")
    other.free()
    X, hists, stats = B.gcr_solve_multi(op, m, jac, Bk, X0, restart=4)  # the refusals left the operator usable
    assert all(s.converged == 1 for s in stats)
    for p in (jac, short):
        p.destroy()
    op.free()


def test_a_workspace_that_does_not_fit_is_refused_with_the_largest_restart(B, capfd):
    """9 000^2 rows at k = 8 and restart 32 ask for 68 block vectors of 5.2 GB: more than the device has. The request is sized against
    the free memory and refused before anything is allocated -- B and X0 are untouched zero pages --, and the sentence names the
    largest restart that fits: held to spmv_amd_gcr_multi_workspace_bytes' arithmetic on the free bytes the sentence reports."""
    n, k, restart = 9000, 8, 32
    rows = n * n
    W = B.gcr_multi_workspace_bytes
    assert W(rows, k, restart, "none") > 350e9
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    pc = B.Precond(op, "none")
    try:
        B.lib().spmv_amd_cg_release_workspace()
        before = _free_bytes()
        capfd.readouterr()
        Bk, X0 = np.zeros((k, rows)), np.zeros((k, rows))  # handed over without the wrapper's copy: never touched, never resident
        cfg, stats = B.CGConfig(2, 1e-6, 0, 0), (B.CGStats * k)()
        rc = B._gcr_multi_lib().spmv_amd_gcr_solve_device_multi(op.op, m.ptr, pc.handle, restart, k, Bk.ctypes.data, X0.ctypes.data, C.byref(cfg), stats)
        assert rc != 0
        err = capfd.readouterr().err
        found = re.search(r"\[GCR-MULTI\] the workspace for 8 systems of 81000000 rows at restart 32 needs ([0-9.]+) GB more, the device has "
                          r"([0-9.]+) GB free: refused \(restart (\d+) is the largest that fits\)", err)
        assert found, err
        free, fits = float(found.group(2)) * 1e9, int(found.group(3))
        assert 1 <= fits < restart
        assert W(rows, k, fits, "none") <= free + 1e8 and W(rows, k, fits + 1, "none") + (65 << 20) >= free - 1e8, (fits, free)
        assert abs(_free_bytes() - before) < (64 << 20)  # nothing was allocated
    finally:
        pc.destroy()
        op.free()
