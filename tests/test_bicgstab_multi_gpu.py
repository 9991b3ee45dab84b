"""Batched BiCGSTAB on the GPU (spmv_amd_bicgstab_solve_device_multi, csrc/bicgstab_multi.hip), through the product library: every
column of every solve BIT for bit (x, history, count, converged) against the numpy restatement on that operator's own product
(tests/bicgstab_multi_restatement.py) -- whole solves on stencil5-csr (row-direct and row-lds), cusparse-csr and stencil7-csr under
both kinds at k = 1, 3 and 8, whose columns stop in different iterations and so exercise freezing; column independence; a poisoned
and a zero neighbour; every end of the loop in one batch; the two-stage sum; determinism and the solve parameters; agreement with the
single-RHS solver; the other solvers' histories; the workspace; the refusals that need a device. The inputs are shown to be sound by
tests/test_bicgstab_multi_host.py, the kernels one by one by tests/test_bicgstab_multi_stages_gpu.py."""
import re

import numpy as np
import pytest

import bicgstab_multi_restatement as BM
from bicgstab_restatement import TABLE, bicgstab, bicgstab_other_rounding, dinv_of, entries_of, hist_err, table_system, third_rounding_bound
from bitwise import same_bits
from test_bicgstab_multi_host import BLOCK_B, BLOCK_CAP, BLOCK_ENDS, BLOCKS

pytestmark = pytest.mark.gpu
ROWLDS_KNOB = "SPMV_AMD_ROWLDS_MIN_GRID"
KS = (1, 3, 8)
# (system, operator, stencil5 form or None)
FORMS = [("grid33", "stencil5-csr", "row-direct"), ("grid33", "stencil5-csr", "row-lds"), ("grid65", "stencil5-csr", "row-direct"),
         ("grid65", "stencil5-csr", "row-lds"), ("grid33", "cusparse-csr", None), ("grid65", "cusparse-csr", None),
         ("cube16", "stencil7-csr", None)]


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_reset_host_matrices()


def grid_of(name):
    rows = table_system(name)[0].shape[0]
    return int(round(rows ** (1.0 / (3 if name.startswith("cube") else 2))))


def open_operator(B, name, mode, form=None, monkeypatch=None):
    A, _, _ = table_system(name)
    if form == "row-lds":
        monkeypatch.setenv(ROWLDS_KNOB, "8")
    m = B.HostMatrix(entries_of(A), A.shape[0], A.shape[0], grid_of(name))
    op = B.Operator(mode)
    assert op.init(m) == 0
    if form is not None:
        assert op.variant() == "stencil5/" + form and op.spmm_variant() == "spmm/stencil5-" + form, (op.variant(), op.spmm_variant())
    return op, m


_products, _restated = {}, {}


def product_of(O, name, mode):
    """The operator's own product: oracle.spmv_stencil5 for stencil5-csr in every form, oracle.spmv_csr for the others."""
    key = (name, mode == "stencil5-csr")
    if key not in _products:
        A, _, _ = table_system(name)
        rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
        grid = grid_of(name)
        _products[key] = (lambda u: O.spmv_stencil5(rp, ci, va, u, grid)) if key[1] else (lambda u: O.spmv_csr(rp, ci, va, u))
    return _products[key]


def restated(O, name, mode, kind, s, tol=BM.TOL, max_iters=1000):
    """The restatement of column s of the system's batch (0: the table system; 1..8: the seeded columns) on the operator's product:
    computed once, shared by every test that needs it."""
    key = (name, mode == "stencil5-csr", kind, s, tol, max_iters)
    if key not in _restated:
        A, b, x0 = table_system(name)
        if s > 0:
            b, x0 = BM.seeded_column(name, s)
        _restated[key] = BM.solve(product_of(O, name, mode), b, x0, dinv_of(A, kind), tol, max_iters)
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


# ---------------------------------------------------------------- whole solves, bit for bit
@pytest.mark.parametrize("kind", ["none", "jacobi"])
@pytest.mark.parametrize("name, mode, form", FORMS, ids=[f"{n}-{f or m}" for n, m, f in FORMS])
def test_whole_solves_bit_for_bit_against_the_restatement(B, O, monkeypatch, name, mode, form, kind):
    """Column 0 is the table system, the rest the seeded columns: they stop between 22 and 36 iterations, by the half step and by the
    whole one, so all but the last spend iterations frozen beside running ones."""
    op, m = open_operator(B, name, mode, form, monkeypatch)
    pc = B.Precond(op, kind)
    try:
        if kind == "jacobi":
            assert same_bits(pc.inverse_diagonal(), dinv_of(table_system(name)[0], kind))
        row = next(r for r in TABLE if r[:3] == (name, kind, BM.TOL))
        for k in KS:
            Bk, X0 = BM.batch(name, k)
            got = B.bicgstab_solve_multi(op, m, pc, Bk, X0)
            for j in range(k):
                want = restated(O, name, mode, kind, j)
                check_column(got, j, want, (name, mode, form, kind, k))
                pinned = (row[3], row[4]) if j == 0 else BM.SEEDED[name][j - 1]
                assert (want[2], want[4]) == pinned and want[3], (name, kind, j, want[2:])
                assert got[2][j].residual_norm == got[1][j][-1]
        assert len({s.iterations for s in got[2]}) >= 4  # k = 8: the columns stop in different iterations
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- independence, bad neighbours
@pytest.mark.parametrize("kind", ["none", "jacobi"])
def test_a_column_has_the_same_bits_in_every_batch(B, O, kind):
    """Seeded column 4 of grid65 alone, in slot 5 of eight and in slot 0 of three: the same x, history and statistics."""
    name = "grid65"
    op, m = open_operator(B, name, "stencil5-csr")
    pc = B.Precond(op, kind)
    try:
        Bk, X0 = BM.batch(name, 8)
        b, x0 = BM.seeded_column(name, 4)
        alone = B.bicgstab_solve_multi(op, m, pc, b[None], x0[None])
        check_column(alone, 0, restated(O, name, "stencil5-csr", kind, 4), "k = 1")
        ids8, ids3 = [0, 1, 2, 3, 5, 4, 6, 7], [4, 0, 7]
        for ids, slot in ((ids8, 5), (ids3, 0)):
            assert ids[slot] == 4
            got = B.bicgstab_solve_multi(op, m, pc, Bk[ids], X0[ids])
            assert same_bits(got[0][slot], alone[0][0]) and same_bits(got[1][slot], alone[1][0]), (len(ids), slot)
            assert stats_tuple(got[2][slot]) == stats_tuple(alone[2][0])
            for s, j in enumerate(ids):
                check_column(got, s, restated(O, name, "stencil5-csr", kind, j), (ids, s))
    finally:
        pc.destroy()
        op.free()


@pytest.mark.parametrize("kind", ["none", "jacobi"])
@pytest.mark.parametrize("mode", ["stencil5-csr", "cusparse-csr"])
def test_a_poisoned_and_a_zero_neighbour(B, O, mode, kind):
    """A column whose b holds an inf: rho = inf, v = A p^ holds NaN, sigma is not finite -- breakdown in iteration 1, history [inf, inf],
    x = x0. A column with b = x0 = 0: sigma = 0, breakdown in iteration 1 with history [0, 0]. In slot 0, slot 1 and the last slot of
    k = 2, 3 and 8 they leave every other column's bits as they are."""
    name = "grid33"
    op, m = open_operator(B, name, mode)
    pc = B.Precond(op, kind)
    try:
        rows = 33 * 33
        healthy_b, healthy_x0 = BM.batch(name, 8)
        poisoned = np.random.default_rng(5).standard_normal(rows)
        poisoned[rows // 2 + 1] = np.inf
        for what, bad, hist in (("inf", poisoned, [np.inf, np.inf]), ("zero", np.zeros(rows), [0.0, 0.0])):
            for k in (2, 3, 8):
                for slot in sorted({0, 1, k - 1}):
                    Bk = np.insert(healthy_b[:k - 1], slot, bad, axis=0)
                    X0 = np.insert(healthy_x0[:k - 1], slot, np.zeros(rows), axis=0)
                    got = B.bicgstab_solve_multi(op, m, pc, Bk, X0)
                    X, hists, stats = got
                    label = (what, k, slot)
                    assert stats[slot].iterations == 1 and stats[slot].converged == 0 and same_bits(hists[slot], hist), (label, hists[slot])
                    assert same_bits(X[slot], np.zeros(rows)), label
                    for j, s in enumerate([s for s in range(k) if s != slot]):
                        check_column(got, s, restated(O, name, mode, kind, j), label)
    finally:
        pc.destroy()
        op.free()


def block_entries(B):
    A = BLOCKS.tocoo()
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row, A.col, A.data
    return e[np.lexsort((e["col"], e["row"]))]


def test_every_end_in_one_batch(B, O, capfd):
    """The 6 x 6 block-diagonal matrix of [[0, 1], [1, 0]], 3 I and 2 I with one column supported on each block: sigma / half / half at
    tol 1e-6 and sigma / an ordinary iteration / omega at tol 0 (tests/test_bicgstab_multi_host.py confirms them on the CPU), each
    column bit for bit, and each breakdown line naming its scalar."""
    e = block_entries(B)
    m = B.HostMatrix(e, 6, 6, -1)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    try:
        rp, ci, va = O.build_csr(e, 6)
        scalar = {"sigma": "sigma = r^.v", "omega": "t.t or t.s"}
        for tol, ends in BLOCK_ENDS.items():
            capfd.readouterr()
            got = B.bicgstab_solve_multi(op, m, pc, BLOCK_B, np.zeros((3, 6)), tol=tol, max_iters=BLOCK_CAP, verbose=1)
            out = capfd.readouterr().out
            lines = [l for l in out.splitlines() if "Breakdown" in l]
            want_lines = [f"[BICGSTAB-MULTI {j}] Breakdown in iteration 1 ({scalar[end]} zero or not finite)" for j, end in enumerate(ends)
                          if end in scalar]
            assert lines == want_lines, out
            assert "[BICGSTAB-MULTI 0] Initial residual: 1.000000e+00 (preconditioner none)" in out and "[PCG" not in out
            for j, end in enumerate(ends):
                want = BM.solve(lambda u: O.spmv_csr(rp, ci, va, u), BLOCK_B[j], np.zeros(6), None, tol, BLOCK_CAP)
                assert want[4] == end, (tol, j, want[4])
                check_column(got, j, want, (tol, j))
                assert got[2][j].iterations == (BLOCK_CAP if end == "max_iters" else 1) and got[2][j].converged == int(end == "half")
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- the two-stage sum
def test_the_two_stage_sum_on_a_1025_grid(B, O):
    """1025^2 rows are 4 105 partials per value: a full slice of 4 096 and a second of 9. One capped solve, k = 2, on the synthetic
    stencil (centre 5, off -1): both columns bit for bit."""
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
        got = B.bicgstab_solve_multi(op, m, pc, Bk, X0, max_iters=cap)
        rp, ci, va = O.stencil5_csr(n)
        for j in range(2):
            want = BM.solve(lambda u: O.spmv_stencil5(rp, ci, va, u, n), Bk[j], X0[j], np.full(rows, 1.0 / 5.0), BM.TOL, cap)
            assert want[2] == cap and not want[3]
            check_column(got, j, want, j)
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- parameters, the single solver, the other histories
def test_solve_parameters_and_the_single_rhs_solver(B, O, capfd):
    """A solve run twice is bit-identical, with the detailed timers too; max_iters = 0 returns x0 and one history entry; a capped
    solve's history is the full one's beginning; verbose changes no bit and tags its lines; every column takes the single-RHS solver's
    count and agrees with it within the row's third-rounding bound; the single solver's and the batched PCG's histories are left alone;
    a from-diagonal handle gives the operator's bits."""
    name, kind, k = "grid65", "jacobi", 3
    A, _, _ = table_system(name)
    op, m = open_operator(B, name, "stencil5-csr")
    pc = B.Precond(op, kind)
    given = B.Precond.from_diagonal(np.asarray(A.diagonal()))
    try:
        Bk, X0 = BM.batch(name, k)
        single = [B.bicgstab_solve(op, m, pc, Bk[j], X0[j]) for j in range(k)]
        _, hp, _ = B.pcg_solve_multi(op, m, pc, Bk[:2], X0[:2], max_iters=3)
        first = B.bicgstab_solve_multi(op, m, pc, Bk, X0)
        again = B.bicgstab_solve_multi(op, m, pc, Bk, X0)
        timed = B.bicgstab_solve_multi(op, m, pc, Bk, X0, timers=1)
        theirs = B.bicgstab_solve_multi(op, m, given, Bk, X0)
        for other in (again, timed, theirs):
            assert same_bits(other[0], first[0]) and all(same_bits(a, c) for a, c in zip(other[1], first[1]))
            assert [stats_tuple(s) for s in other[2]] == [stats_tuple(s) for s in first[2]]
        st, stt = first[2][0], timed[2][0]
        assert st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0
        assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0
        assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms
        # the single-RHS solver: the same count, another rounding of the sums
        # (column 0: the table's stored figure; a seeded column: twice what the two CPU roundings disagree by on it, as the table stores)
        for j in range(k):
            x, h, s = single[j]
            stored = next(r for r in TABLE if r[:3] == (name, kind, BM.TOL))[5]
            if j > 0:
                d = dinv_of(A, kind)
                stored = 2.0 * hist_err(bicgstab(A, Bk[j], X0[j], d, BM.TOL)[1], bicgstab_other_rounding(A, Bk[j], X0[j], d, BM.TOL)[1])
            bound = third_rounding_bound(stored)
            assert first[2][j].iterations == s.iterations and first[2][j].converged == s.converged == 1, j
            err = hist_err(first[1][j], h)
            print(f"column {j}: batched against single-RHS {err:.2e} (bound {bound:.0e})")
            assert err <= bound and np.max(np.abs(first[0][j] - x)) <= bound * np.max(np.abs(x)), (j, err)
        # the other solvers' histories are left alone
        L = B._pcg_lib()
        hs = np.zeros(len(single[-1][1]) + 1)
        assert L.spmv_amd_bicgstab_last_history(hs.ctypes.data, len(hs)) == len(single[-1][1]) and same_bits(hs[:-1], single[-1][1])
        for j in range(2):
            hm = np.zeros(8)
            assert L.spmv_amd_pcg_last_history_multi(j, hm.ctypes.data, 8) == len(hp[j]) and same_bits(hm[:len(hp[j])], hp[j])
        # max_iters 0 and a cap
        Xz, hz, sz = B.bicgstab_solve_multi(op, m, pc, Bk, X0, max_iters=0)
        X5, h5, s5 = B.bicgstab_solve_multi(op, m, pc, Bk, X0, max_iters=5)
        for j in range(k):
            assert sz[j].iterations == 0 and sz[j].converged == 0 and same_bits(Xz[j], X0[j]) and same_bits(hz[j], first[1][j][:1])
            assert s5[j].iterations == 5 and s5[j].converged == 0 and same_bits(h5[j], first[1][j][:6]) and s5[j].residual_norm == h5[j][0]
            check_column((X5, h5, s5), j, restated(O, name, "stencil5-csr", kind, j, max_iters=5), ("cap", j))
        # a history cap smaller than the count, and a column that is not there
        few = np.full(5, -1.0)
        LM = B._bicgstab_multi_lib()
        assert LM.spmv_amd_bicgstab_last_history_multi(0, few.ctypes.data, 3) == 6 and same_bits(few[:3], h5[0][:3]) and few[3] == -1.0
        assert LM.spmv_amd_bicgstab_last_history_multi(k, few.ctypes.data, 3) == -1
        # verbose
        capfd.readouterr()
        loud = B.bicgstab_solve_multi(op, m, pc, Bk, X0, max_iters=5, verbose=2)
        out = capfd.readouterr().out
        assert same_bits(loud[0], X5) and all(same_bits(a, c) for a, c in zip(loud[1], h5))
        assert len(re.findall(r"\[BICGSTAB-MULTI \d\] Iter +\d+: residual", out)) == 5 * k
        assert out.count("Initial residual") == k and "(preconditioner jacobi)" in out and "[PCG" not in out and "[BICGSTAB-DEVICE]" not in out
        assert "[BICGSTAB-MULTI] 3 systems, time breakdown (whole batch):" in out and "Breakdown" not in out
        assert [s.residual_norm for s in loud[2]] == [h[5] for h in h5]
    finally:
        pc.destroy(), given.destroy()
        op.free()


# ---------------------------------------------------------------- workspace
def test_workspace_is_counted_and_released_with_the_others(B):
    name, k = "grid65", 4
    rows = 65 * 65
    op, m = open_operator(B, name, "stencil5-csr")
    none, jac = B.Precond(op, "none"), B.Precond(op, "jacobi")
    try:
        Bk, X0 = BM.batch(name, k)
        B.lib().spmv_amd_cg_release_workspace()
        assert B.bicgstab_multi_workspace_bytes() == 0
        first = B.bicgstab_solve_multi(op, m, none, Bk, X0)
        six = B.bicgstab_multi_workspace_bytes()
        assert 6 * k * rows * 8 <= six < 1.2 * 6 * k * rows * 8  # X, R, r^0, P, V, T and the small arrays
        B.bicgstab_solve_multi(op, m, jac, Bk, X0)
        eight = B.bicgstab_multi_workspace_bytes()
        assert eight - six == 2 * k * rows * 8  # P^ and S^ join for kind "jacobi" only
        assert B._pcg_lib().spmv_amd_pcg_multi_workspace_bytes() == 0  # the batched PCG workspace is another one
        for release in (B.lib().spmv_amd_cg_release_workspace, B._pcg_lib().spmv_amd_pcg_release_workspace):
            release()
            assert B.bicgstab_multi_workspace_bytes() == 0
            again = B.bicgstab_solve_multi(op, m, none, Bk, X0)
            assert same_bits(again[0], first[0]) and B.bicgstab_multi_workspace_bytes() == six
        B.bicgstab_solve_multi(op, m, none, Bk[:2], X0[:2])  # another k: the workspace is made anew
        assert B.bicgstab_multi_workspace_bytes() < six
        op.free()
        assert B.bicgstab_multi_workspace_bytes() == 0
    finally:
        none.destroy(), jac.destroy()
        op.free()


# ---------------------------------------------------------------- refusals that need a device
def test_refusals_that_need_a_device(B, capfd):
    name = "grid33"
    rows = 33 * 33
    A, _, _ = table_system(name)
    op, m = open_operator(B, name, "stencil5-csr")
    Bk, X0 = BM.batch(name, 2)

    def refused(handle, word, operator=None, matrix=None):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            B.bicgstab_solve_multi(operator or op, matrix or m, handle, Bk, X0)
        err = capfd.readouterr().err
        assert "[BICGSTAB-MULTI]" in err and word in err, err

    for make, word in ((lambda: B.Precond.chebyshev(op, 2), "chebyshev"), (lambda: B.Precond.multigrid(op), "multigrid"),
                       (lambda: B.Precond.multigrid_multi(op, max_rhs=4), "multigrid")):
        pc = make()
        refused(pc, word)
        refused(pc, "symmetric definite")
        pc.destroy()
    jac = B.Precond(op, "jacobi")
    B.bicgstab_solve_multi(op, m, jac, Bk, X0)
    other = B.Operator("cusparse-csr")
    assert other.init(m) == 0
    refused(jac, "refused", operator=other)  # a handle of another operator
    small = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows - 1, rows - 1, -1)
    refused(jac, "square system of that size", matrix=small)
    short = B.Precond.from_diagonal(np.ones(rows - 1))
    refused(short, "the preconditioner is for")
    other.free()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
    m2 = B.HostMatrix(entries_of(A), rows, rows, 33)
    assert op.init(m2) == 0
    refused(jac, "refused", matrix=m2)  # a handle from before the re-init
    fresh = B.Precond(op, "jacobi")
    X, hists, stats = B.bicgstab_solve_multi(op, m2, fresh, Bk, X0)  # the refusals left the operator usable
    assert all(s.converged == 1 for s in stats)
    for p in (jac, short, fresh):
        p.destroy()
    op.free()
