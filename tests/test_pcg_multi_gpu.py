"""Batched preconditioned CG on the GPU (spmv_amd_pcg_solve_device_multi, csrc/pcg_multi.hip), through the product library: whole
solves bit for bit against the numpy restatement (tests/pcg_multi_restatement.py: iterations, verdict, history and x), column by
column against spmv_amd_pcg_solve_device at the project's 1e-10, kind "none" bit for bit against spmv_amd_cg_solve_device_multi,
stencil7-csr through spmm/csr, column independence, mixed batches with columns that stop at different iterations or break down,
the solve parameters, the refusals that need a device, and the workspace. The systems are rows of chebyshev_restatement.TABLE that
tests/test_pcg_multi_host.py shows to be honest in the batched dot shape."""
import functools

import numpy as np
import pytest

import chebyshev_restatement as CH
import multi_rhs_restatement as M
import pcg_multi_restatement as PM
import pcg_restatement as P
import stencil7 as S7
from bitwise import same_bits
from conftest import hist_err
from test_multi_rhs_gpu import (check_print_out, check_verbose_changes_nothing_else, columns, eigenmode, expected_print_out, printed,
                                stats_tuple)

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the project's own (tests/test_multi_rhs_gpu.py)
# (system, kind, degree) of the whole-solve tests
ROWS = [("negated65", "jacobi", None), ("scaled127", "jacobi", None), ("plain127", "none", None), ("scaled127", "chebyshev", 2),
        ("scaled127", "chebyshev", 4), ("poisson127", "chebyshev", 4)]
WIDE = [("plain601", "jacobi", None), ("scaled601", "jacobi", None), ("scaled601", "chebyshev", 2)]  # 601 columns: a short last block
FORMS = [("stencil5-csr", "row-lds"), ("stencil5-csr", "row-direct"), ("cusparse-csr", None)]


def row_id(row):
    return "-".join(str(v) for v in row if v is not None)


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


@functools.lru_cache(maxsize=4)
def system(name):
    """A, its entries, grid and a batch of four columns: the table's own (b, x0), ones from zero, a random pair, and twice the first."""
    A, b, x0 = CH.table_system(name)
    N = len(b)
    rng = np.random.default_rng(N + len(name))
    Bk = np.stack([b, np.ones(N), rng.standard_normal(N), 2.0 * b])
    X0 = np.stack([x0, np.zeros(N), rng.standard_normal(N), 2.0 * x0])
    return A, P.entries_of(A), int(round(np.sqrt(N))), Bk, X0


def open_operator(B, mode, variant, e, rows, grid):
    m = B.HostMatrix(e, rows, rows, grid)
    op = B.Operator(mode)
    assert op.init(m) == 0
    if variant is not None:
        assert op.select_variant(variant) == 0 and op.spmm_variant() == "spmm/stencil5-" + variant
    return op, m


def close_operator(op, variant):
    if variant is not None:
        op.select_variant(None)
    op.free()


def make_precond(B, op, kind, degree):
    if kind == "chebyshev":
        return B.Precond.chebyshev(op, degree)
    return B.Precond(op, kind)


def precond_data(pc, kind):
    """dinv and the coefficients as the library holds them (None where the kind has none)."""
    if kind == "none":
        return None, None
    return pc.inverse_diagonal(), (None if kind == "jacobi" else list(pc.chebyshev_info()[3]))


def product_and_layout(O, mode, e, rows, grid):
    rp, ci, va = O.build_csr(e, rows)
    if mode == "stencil5-csr":
        return (lambda v: O.spmv_stencil5(rp, ci, va, v, grid)), M.grid(grid)
    return (lambda v: O.spmv_csr(rp, ci, va, v)), M.flat()


_restated = {}


def restated(O, name, kind, degree, mode, dinv, coef):
    """The restatement of the batch's four columns (the product and the p.Ap layout differ between the two operators, not between the
    stencil variants): computed once."""
    key = (name, kind, degree, mode == "stencil5-csr")
    if key not in _restated:
        A, e, grid, Bk, X0 = system(name)
        matvec, layout = product_and_layout(O, mode, e, A.shape[0], grid)
        _restated[key] = [PM.solve(matvec, layout, Bk[j], X0[j], dinv, coef) for j in range(len(Bk))]
    return _restated[key]


def check_bits(got, want, label):
    X, hists, stats = got
    for j, (x, hist, its, converged, breakdown) in enumerate(want):
        assert stats[j].iterations == its and stats[j].converged == int(converged), (label, j, stats[j].iterations, its)
        assert same_bits(hists[j], hist), (label, j)
        assert same_bits(X[j], x), (label, j, int(np.sum(X[j] != x)))


# ---------------------------------------------------------------- whole solves, bit for bit
@pytest.mark.parametrize("mode, variant", FORMS, ids=[v or m for m, v in FORMS])
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_whole_solves_bit_for_bit_against_the_restatement(B, O, row, mode, variant):
    name, kind, degree = row
    A, e, grid, Bk, X0 = system(name)
    op, m = open_operator(B, mode, variant, e, A.shape[0], grid)
    pc = make_precond(B, op, kind, degree)
    try:
        dinv, coef = precond_data(pc, kind)
        if dinv is not None:
            assert same_bits(dinv, 1.0 / P.diagonal(A))
        want = restated(O, name, kind, degree, mode, dinv, coef)
        got = B.pcg_solve_multi(op, m, pc, Bk, X0)
        check_bits(got, want, row)
        table = {(n, d): its for n, d, tol, its in CH.TABLE if tol == 1e-6}
        assert got[2][0].iterations == table[(name, degree)] and got[2][0].converged == 1  # the table's own column
        assert got[2][3].iterations == got[2][0].iterations and same_bits(got[0][3], 2.0 * got[0][0])  # scaling by 2 is exact
        again = B.pcg_solve_multi(op, m, pc, Bk, X0)
        assert same_bits(again[0], got[0]) and all(same_bits(a, c) for a, c in zip(again[1], got[1]))
    finally:
        pc.destroy()
        close_operator(op, variant)


# ---------------------------------------------------------------- against the single-RHS solver
@pytest.mark.parametrize("row", ROWS + WIDE, ids=row_id)
def test_against_the_single_rhs_solver(B, row):
    """Column by column: equal iteration counts and verdicts, history and x to 1e-10 (the two solvers sum in different shapes)."""
    name, kind, degree = row
    A, e, grid, Bk, X0 = system(name)
    op, m = open_operator(B, "stencil5-csr", None, e, A.shape[0], grid)
    pc = make_precond(B, op, kind, degree)
    try:
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        for j in range(len(Bk)):
            x, h, st = B.pcg_solve_device(op, m, pc, Bk[j], X0[j])
            assert stats[j].iterations == st.iterations and stats[j].converged == st.converged == 1, (row, j)
            assert len(hists[j]) == len(h) and hist_err(hists[j], h) < TOL, (row, j)
            assert np.max(np.abs(X[j] - x)) <= TOL * np.max(np.abs(x)), (row, j)
            assert abs(stats[j].residual_norm - st.residual_norm) <= TOL * st.residual_norm
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- kind "none" is the batched CG solver
def test_kind_none_is_batched_cg_bit_for_bit(B, O):
    n = 127
    N = n * n
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    try:
        Bk, X0 = columns(n)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        Xc, hc, sc = B.cg_solve_multi(op, m, Bk, X0)
        for j in range(len(Bk)):
            assert same_bits(X[j], Xc[j]) and same_bits(hists[j], hc[j]), j
            assert stats_tuple(stats[j]) == stats_tuple(sc[j]), j
        assert stats[2].iterations == 1  # the eigenmode: frozen from iteration 2 on
    finally:
        pc.destroy()
        op.free()


def stencil7_batch(n, center):
    N = n ** 3
    rng = np.random.default_rng(31 * n + int(center))
    return S7.coo(n, center=center, off=-1.0), np.stack([rng.standard_normal(N), np.ones(N), rng.standard_normal(N)]), \
        np.stack([rng.standard_normal(N), np.zeros(N), np.zeros(N)])


def test_kind_none_is_batched_cg_on_stencil7(B):
    n = 20
    e, Bk, X0 = stencil7_batch(n, 7.0)
    m = B.HostMatrix(e, n ** 3, n ** 3, n)
    op = B.Operator("stencil7-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    try:
        assert op.spmm_variant() == "spmm/csr"
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        Xc, hc, sc = B.cg_solve_multi(op, m, Bk, X0)
        for j in range(len(Bk)):
            assert same_bits(X[j], Xc[j]) and same_bits(hists[j], hc[j]) and stats_tuple(stats[j]) == stats_tuple(sc[j]), j
    finally:
        pc.destroy()
        op.free()


@pytest.mark.parametrize("kind, degree", [("jacobi", None), ("chebyshev", 2)])
@pytest.mark.parametrize("center", [7.0, 6.0])
@pytest.mark.parametrize("n", [20, 33])
def test_stencil7_against_the_restatement(B, O, n, center, kind, degree):
    N = n ** 3
    e, Bk, X0 = stencil7_batch(n, center)
    rp, ci, va = O.build_csr(e, N)
    m = B.HostMatrix(e, N, N, n)
    op = B.Operator("stencil7-csr")
    assert op.init(m) == 0
    pc = make_precond(B, op, kind, degree)
    try:
        dinv, coef = precond_data(pc, kind)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        for j in range(len(Bk)):
            x, hist, its, converged, _ = PM.solve(lambda v: O.spmv_csr(rp, ci, va, v), M.flat(), Bk[j], X0[j], dinv, coef)
            assert stats[j].iterations == its and stats[j].converged == int(converged) == 1, (j, stats[j].iterations, its)
            assert len(hists[j]) == len(hist) and hist_err(hists[j], hist) < TOL, j
            assert np.max(np.abs(X[j] - x)) <= TOL * np.max(np.abs(x)), j
    finally:
        pc.destroy()
        op.free()


def test_a_from_diagonal_preconditioner_gives_the_operators_bits(B):
    A, e, grid, Bk, X0 = system("scaled127")
    op, m = open_operator(B, "stencil5-csr", None, e, A.shape[0], grid)
    own, given = B.Precond(op, "jacobi"), B.Precond.from_diagonal(P.diagonal(A))
    try:
        X, hists, stats = B.pcg_solve_multi(op, m, own, Bk, X0)
        Xd, hd, sd = B.pcg_solve_multi(op, m, given, Bk, X0)
        assert same_bits(X, Xd) and all(same_bits(a, c) for a, c in zip(hists, hd))
        assert [stats_tuple(s) for s in stats] == [stats_tuple(s) for s in sd]
    finally:
        own.destroy(), given.destroy()
        op.free()


# ---------------------------------------------------------------- independence
@pytest.mark.parametrize("kind, degree", [("jacobi", None), ("chebyshev", 2)])
def test_columns_are_independent_bit_for_bit(B, kind, degree):
    """Permuted columns, and one column at every k = 1..8 and in every slot: the same x, history and statistics."""
    A, e, grid, _, _ = system("scaled127")
    N = A.shape[0]
    op, m = open_operator(B, "stencil5-csr", None, e, N, grid)
    pc = make_precond(B, op, kind, degree)
    try:
        rng = np.random.default_rng(11)
        base = rng.standard_normal(N)
        Bk = np.stack([base, np.ones(N), eigenmode(grid), rng.standard_normal(N), 2.0 * base, np.ones(N) + 0.01 * np.sin(np.arange(N)),
                       rng.uniform(0, 1, N), 0.5 * np.ones(N)])
        X0 = np.zeros_like(Bk)
        X0[3] = rng.standard_normal(N)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        assert len({s.iterations for s in stats}) > 1  # columns stop at different iterations
        perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
        Xp, hp, sp_ = B.pcg_solve_multi(op, m, pc, Bk[perm], X0[perm])
        for slot, j in enumerate(perm):
            assert same_bits(Xp[slot], X[j]) and same_bits(hp[slot], hists[j]) and stats_tuple(sp_[slot]) == stats_tuple(stats[j]), (slot, j)
        for k in range(1, 9):
            for slot in range(k):  # column 3 in slot `slot` of k, the others around it
                ids = [(3 - slot + i) % 8 for i in range(k)]
                assert ids[slot] == 3
                Xk, hk, sk = B.pcg_solve_multi(op, m, pc, Bk[ids], X0[ids])
                for s, j in enumerate(ids):
                    assert same_bits(Xk[s], X[j]) and same_bits(hk[s], hists[j]) and stats_tuple(sk[s]) == stats_tuple(stats[j]), (k, slot, s)
        assert same_bits(hists[4], 2.0 * hists[0]) and same_bits(X[4], 2.0 * X[0])
    finally:
        pc.destroy()
        op.free()


@pytest.mark.parametrize("kind, degree", [("jacobi", None), ("chebyshev", 2), ("none", None)])
def test_a_mixed_batch_and_bad_columns(B, kind, degree):
    """An eigenmode (one iteration), ones and a random column stop at different iterations. A column with b = 0 and one with a NaN
    report what spmv_amd_pcg_solve_device reports for that column alone (iterations, converged = 0) in slot 0, slot 1 and the last
    slot, and leave their neighbours' bits unchanged."""
    n = 127
    A = P.stencil5(n)
    N = n * n
    op, m = open_operator(B, "stencil5-csr", None, P.entries_of(A), N, n)
    pc = make_precond(B, op, kind, degree)
    try:
        rng = np.random.default_rng(17)
        healthy = np.stack([eigenmode(n), np.ones(N), rng.standard_normal(N), rng.uniform(0, 1, N), rng.standard_normal(N)])
        one_nan = rng.standard_normal(N)
        one_nan[N // 2 + 1] = np.nan
        zeros = np.zeros_like(healthy)
        Xh, hh, sh = B.pcg_solve_multi(op, m, pc, healthy, zeros)
        assert all(s.converged == 1 for s in sh) and len({s.iterations for s in sh}) >= 2
        if kind != "chebyshev":
            assert sh[0].iterations == 1  # the eigenmode
        for what, bad in (("zero", np.zeros(N)), ("nan", one_nan)):
            _, hb, sb = B.pcg_solve_device(op, m, pc, bad, np.zeros(N))
            assert sb.converged == 0, what
            for k in (2, 5, 6):
                for slot in sorted({0, 1, k - 1}):
                    Bk = np.insert(healthy[:k - 1], slot, bad, axis=0)
                    X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, np.zeros((k, N)))
                    assert stats[slot].iterations == sb.iterations and stats[slot].converged == 0, (what, k, slot, stats[slot].iterations)
                    assert len(hists[slot]) == len(hb), (what, k, slot)
                    for j, s in enumerate([s for s in range(k) if s != slot]):
                        assert same_bits(X[s], Xh[j]) and same_bits(hists[s], hh[j]) and stats_tuple(stats[s]) == stats_tuple(sh[j]), (what, k, slot, s)
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- the print-out
def test_print_out_under_jacobi(B, O, capfd):
    """A 32 x 32 system with k = 3 (odd k: 8-byte accesses) whose middle column has a zero right-hand side (p.Ap = r.z = 0: breakdown in
    iteration 1): the whole print-out of a solve under verbose 1, and under verbose 2 with max_iters = 5, line for line -- the kind on
    the initial lines, a Breakdown line for the zero column and for no other; printing changes no bit of what the solve returns."""
    n = 32
    N = n * n
    op, m = open_operator(B, "stencil5-csr", None, O.stencil5_coo(n), N, n)
    pc = B.Precond(op, "jacobi")
    try:
        Bk = np.stack([np.ones(N), np.zeros(N), np.random.default_rng(32).standard_normal(N)])
        X0 = np.zeros((3, N))
        for verbose, kw in ((1, {}), (2, {"max_iters": 5})):
            silent = B.pcg_solve_multi(op, m, pc, Bk, X0, **kw)
            printed(capfd)
            loud = B.pcg_solve_multi(op, m, pc, Bk, X0, verbose=verbose, **kw)
            got = printed(capfd)
            check_verbose_changes_nothing_else(silent, loud, verbose)
            check_print_out(got, expected_print_out("PCG-MULTI", loud[1], loud[2], verbose, " (preconditioner jacobi)", breakdown=(1,)))
            assert [l for l in got if "Breakdown" in l] == ["[PCG-MULTI 1] Breakdown in iteration 1 (pAp or r.z zero or not finite)"]
            assert len([l for l in got if " Iter " in l]) == (0 if verbose == 1 else 5 + 1 + 5)
            assert [s.converged for s in loud[2]] == ([1, 0, 1] if verbose == 1 else [0, 0, 0])
            assert [s.iterations for s in loud[2]][1] == 1 and len(loud[1][1]) == 2
    finally:
        pc.destroy()
        op.free()


# ---------------------------------------------------------------- solve parameters
def test_solve_parameters(B, O):
    name, kind, degree = "scaled127", "jacobi", None
    A, e, grid, Bk, X0 = system(name)
    N = A.shape[0]
    op, m = open_operator(B, "stencil5-csr", None, e, N, grid)
    pc = make_precond(B, op, kind, degree)
    cheb = make_precond(B, op, "chebyshev", 2)
    try:
        dinv, _ = precond_data(pc, kind)
        X, hists, stats = B.pcg_solve_multi(op, m, pc, Bk, X0)
        # max_iters 0: the initial residual alone, x0 back; max_iters 1: one iteration of the full solve
        Xz, hz, sz = B.pcg_solve_multi(op, m, pc, Bk, X0, max_iters=0)
        X1, h1, s1 = B.pcg_solve_multi(op, m, pc, Bk, X0, max_iters=1)
        for j in range(len(Bk)):
            assert sz[j].iterations == 0 and sz[j].converged == 0 and same_bits(Xz[j], X0[j]) and same_bits(hz[j], hists[j][:1])
            assert sz[j].residual_norm == hists[j][0]
            assert s1[j].iterations == 1 and s1[j].converged == 0 and same_bits(h1[j], hists[j][:2]) and s1[j].residual_norm == hists[j][0]
        # tol 1e-10: the table's count for column 0, the history continues the 1e-6 one bit for bit
        Xt, ht, st = B.pcg_solve_multi(op, m, pc, Bk, X0, tol=1e-10)
        assert st[0].iterations == 31 and st[0].converged == 1 and same_bits(ht[0][:len(hists[0])], hists[0])
        want = restated(O, name, kind, degree, "stencil5-csr", dinv, None)
        assert same_bits(hists[0], want[0][1])
        # detailed timers change no bit, and fill the breakdown
        for handle in (pc, cheb):
            plain = B.pcg_solve_multi(op, m, handle, Bk, X0)
            timed = B.pcg_solve_multi(op, m, handle, Bk, X0, timers=1)
            assert same_bits(plain[0], timed[0]) and all(same_bits(a, c) for a, c in zip(plain[1], timed[1]))
            t = timed[2][0]
            assert t.time_spmv_ms > 0 and t.time_blas1_ms > 0 and t.time_reductions_ms > 0
            assert t.time_spmv_ms + t.time_blas1_ms + t.time_reductions_ms <= t.time_total_ms
            assert plain[2][0].time_spmv_ms == 0 and plain[2][0].time_total_ms > 0
        # a history cap smaller than the count: the caller gets `cap` entries and the full length
        few = np.full(5, -1.0)
        assert B._pcg_lib().spmv_amd_pcg_last_history_multi(0, few.ctypes.data, 3) == len(timed[1][0])
        assert same_bits(few[:3], timed[1][0][:3]) and few[3] == -1.0
        assert B._pcg_lib().spmv_amd_pcg_last_history_multi(len(Bk), few.ctypes.data, 3) == -1
    finally:
        pc.destroy(), cheb.destroy()
        op.free()


# ---------------------------------------------------------------- refusals that need a device
def test_refusals_that_need_a_device(B, capfd):
    n = 32
    A = P.scaled_stencil5(n, 1, 4)
    rows = n * n
    e = P.entries_of(A)
    op, m = open_operator(B, "stencil5-csr", None, P.entries_of(P.stencil5(n)), rows, n)
    Bk, X0 = np.ones((2, rows)), np.zeros((2, rows))

    def refused(handle, word, operator=None, matrix=None):
        with pytest.raises(RuntimeError):
            B.pcg_solve_multi(operator or op, matrix or m, handle, Bk, X0)
        err = capfd.readouterr().err
        assert "[PCG-MULTI]" in err and word in err, err

    mg = B.Precond.multigrid(op)
    refused(mg, "multigrid")
    mg.destroy()
    jac = B.Precond(op, "jacobi")
    B.pcg_solve_multi(op, m, jac, Bk, X0)
    other = B.Operator("cusparse-csr")
    assert other.init(m) == 0
    refused(jac, "refused", operator=other)                    # a handle of another operator
    theirs = B.Precond(other, "jacobi")
    refused(theirs, "refused")
    small = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows - 1, rows - 1, -1)
    refused(jac, "square system of that size", matrix=small)
    short = B.Precond.from_diagonal(np.ones(rows - 1))
    refused(short, "the preconditioner is for")
    other.free()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
    m2 = B.HostMatrix(e, rows, rows, n)
    assert op.init(m2) == 0
    refused(jac, "refused", matrix=m2)                          # a handle from before the re-init
    fresh = B.Precond(op, "jacobi")
    X, hists, stats = B.pcg_solve_multi(op, m2, fresh, Bk, X0)    # the refusals left the operator usable
    assert all(s.converged == 1 for s in stats)
    for p in (jac, theirs, short, fresh):
        p.destroy()
    op.free()


# ---------------------------------------------------------------- workspace
def test_workspace_is_counted_released_and_shared_in_turn(B):
    A, e, grid, Bk, X0 = system("scaled127")
    N = A.shape[0]
    L = B._pcg_lib()
    op, m = open_operator(B, "stencil5-csr", None, e, N, grid)
    jac, cheb = B.Precond(op, "jacobi"), B.Precond.chebyshev(op, 2)
    try:
        assert L.spmv_amd_pcg_multi_workspace_bytes() == 0
        first = B.pcg_solve_multi(op, m, jac, Bk, X0)
        four = L.spmv_amd_pcg_multi_workspace_bytes()
        assert 4 * 4 * N * 8 <= four < 1.2 * 4 * 4 * N * 8
        B.pcg_solve_multi(op, m, cheb, Bk, X0)
        six = L.spmv_amd_pcg_multi_workspace_bytes()
        assert six - four == 2 * 4 * N * 8  # D and Z join for the Chebyshev kind only
        for release in (B.lib().spmv_amd_cg_release_workspace, L.spmv_amd_pcg_release_workspace):
            release()
            assert L.spmv_amd_pcg_multi_workspace_bytes() == 0
            again = B.pcg_solve_multi(op, m, jac, Bk, X0)
            assert same_bits(again[0], first[0]) and L.spmv_amd_pcg_multi_workspace_bytes() == four
        # the four solvers in turn on one operator, twice: each reproduces its own bits
        runs = []
        for _ in range(2):
            cg = B.cg_solve(op, m, Bk[0], X0[0], device=True)
            multi = B.cg_solve_multi(op, m, Bk, X0, max_iters=40)
            single = B.pcg_solve_device(op, m, jac, Bk[0], X0[0])
            batched = B.pcg_solve_multi(op, m, jac, Bk, X0)
            runs.append((cg[0], cg[1], multi[0], np.concatenate(multi[1]), single[0], single[1], batched[0], np.concatenate(batched[1])))
        assert all(same_bits(a, c) for a, c in zip(*runs))
        assert same_bits(runs[0][6], first[0])
        assert hist_err(runs[0][7][:len(runs[0][5])], runs[0][5]) < TOL  # column 0 of the batch is the single solve's system
        op.free()
        assert L.spmv_amd_pcg_multi_workspace_bytes() == 0 and B._multi_lib().spmv_amd_cg_multi_workspace_bytes() == 0
    finally:
        jac.destroy(), cheb.destroy()
        op.free()
