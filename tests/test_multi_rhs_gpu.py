"""Several right-hand sides per matrix pass on the GPU: the SpMM (spmv_amd_spmm_device) against the CPU oracle column by column,
bit for bit, through every kernel variant of both operators that have the path; the batched CG (spmv_amd_cg_solve_device_multi)
against oracle_cg on every column; the columns' independence (permutation, k, scaling: bit for bit); and the coexistence of the
batched solver with cg_solve_device on one operator."""
import ctypes
import os

import numpy as np
import pytest

import matrices as M
from conftest import GOLDEN, hist_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
KS = list(range(1, 9))  # every instantiation of the kernel templates


def random_stencil(O, n, seed):
    rng = np.random.default_rng(seed)
    e = O.stencil5_coo(n)
    e["value"] = rng.uniform(-3.0, 3.0, len(e))
    return e


@pytest.mark.parametrize("n", [3, 81, 200, 512, 700])
def test_spmm_stencil_bit_exact_every_variant_and_k(B, O, fresh_host_matrices, n):
    e = random_stencil(O, n, 100 + n)
    rows = n * n
    rp, ci, va = O.build_csr(e, rows)
    m = B.HostMatrix(e, rows, rows, n)
    rng = np.random.default_rng(n)
    X = rng.standard_normal((8, rows))
    want_st = np.stack([O.spmv_stencil5(rp, ci, va, X[j], n) for j in range(8)])
    want_csr = np.stack([O.spmv_csr(rp, ci, va, X[j]) for j in range(8)])
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    for forced in ("row-lds", "row-direct", "row-generic", None):
        op.select_variant(forced)
        single = [op.run_timed(X[j])[0] for j in range(3)]
        for k in KS:
            Y = op.run_spmm(X[:k])
            for j in range(k):
                assert np.array_equal(Y[j], want_st[j]), (forced, k, j)
            for j in range(min(k, 3)):  # column j == the single-vector product of column j
                assert np.array_equal(Y[j], single[j]), (forced, k, j)
        if forced is not None and n >= 2:
            assert op.spmm_variant() == "spmm/stencil5-" + forced
    op.select_variant(None)
    op.free()
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    assert op.spmm_variant() == "spmm/csr"
    for k in KS:
        Y = op.run_spmm(X[:k])
        for j in range(k):
            assert np.array_equal(Y[j], want_csr[j]), (k, j)
    op.free()


@pytest.mark.parametrize("fixture", ["stencil_9point", "banded", "dense_blocks", "ill_conditioned"])
def test_spmm_structured_non_stencil_matrices(B, O, fresh_host_matrices, fixture):
    e, rows, cols, _ = {"stencil_9point": lambda: M.stencil_9point(60), "banded": lambda: M.banded(3000, 7),
                        "dense_blocks": lambda: M.dense_blocks(1500, 37), "ill_conditioned": lambda: M.ill_conditioned(2000)}[fixture]()
    grid = 60 if fixture == "stencil_9point" else -1
    rp, ci, va = O.build_csr(e, rows)
    X = np.random.default_rng(7).standard_normal((8, cols))
    want = np.stack([O.spmv_csr(rp, ci, va, X[j]) for j in range(8)])
    m = B.HostMatrix(e, rows, cols, grid)
    for mode in ("stencil5-csr", "cusparse-csr"):
        op = B.Operator(mode)
        assert op.init(m) == 0
        if mode == "stencil5-csr":
            assert op.spmm_variant() == "spmm/stencil5-row-generic(csr-loop)"
        for k in KS:
            Y = op.run_spmm(X[:k])
            for j in range(k):
                assert np.array_equal(Y[j], want[j]), (mode, k, j)
        op.free()


def eigenmode(n):
    s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
    return np.outer(s, s).ravel()


def columns(n, seed=1):
    rng = np.random.default_rng(seed)
    N = n * n
    Bk = np.stack([np.ones(N), rng.standard_normal(N), eigenmode(n), np.ones(N)])
    X0 = np.zeros((4, N))
    X0[3] = rng.standard_normal(N)
    return Bk, X0


def check_against_oracle(O, rp, ci, va, grid, Bk, X0, X, hists, stats, max_iters=1000):
    for j in range(Bk.shape[0]):
        xo, ho, ro = O.cg(rp, ci, va, grid, Bk[j], X0[j], max_iters=max_iters)
        st = stats[j]
        assert st.iterations == ro.iterations and st.converged == ro.converged, (j, st.iterations, ro.iterations)
        assert len(hists[j]) == len(ho) and hist_err(hists[j], ho) < TOL, j
        assert np.max(np.abs(X[j] - xo)) <= TOL * np.max(np.abs(xo)), j
        assert abs(st.solution_sum - ro.solution_sum) <= TOL * max(abs(ro.solution_sum), 1e-300) + 1e-12 * ro.solution_norm, j
        assert abs(st.solution_norm - ro.solution_norm) <= TOL * ro.solution_norm, j
        if ro.residual_norm > 1e-13 * ro.b_norm:
            assert abs(st.residual_norm - ro.residual_norm) <= TOL * ro.residual_norm, j
        else:  # exact convergence (the eigenmode): rounding noise on both sides, compared as hist_err does
            assert st.residual_norm <= 1e-12 * ro.b_norm, j


@pytest.mark.parametrize("n", [81, 200, 512])
def test_cg_multi_matches_oracle_per_column(B, O, fresh_host_matrices, n):
    m = B.HostMatrix(O.stencil5_coo(n), n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    Bk, X0 = columns(n)
    X, hists, stats = B.cg_solve_multi(op, m, Bk, X0)
    rp, ci, va = O.stencil5_csr(n)
    check_against_oracle(O, rp, ci, va, n, Bk, X0, X, hists, stats)
    assert stats[2].iterations == 1  # the eigenmode converges in one iteration
    assert len({s.time_total_ms for s in stats}) == 1 and stats[0].time_total_ms > 0
    op.free()


def test_cg_multi_cusparse_csr_on_symmetric_file(B, O, fresh_host_matrices):
    m = B.load_matrix_market(os.path.join(GOLDEN, "sym_spd40.mtx"))
    rows = m.c.rows
    rp, ci, va = O.build_csr(m.entries, rows)
    rng = np.random.default_rng(5)
    Bk = np.stack([np.ones(rows), rng.standard_normal(rows), 3.0 * np.ones(rows), np.ones(rows)])
    X0 = np.zeros((4, rows))
    X0[3] = rng.standard_normal(rows)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    X, hists, stats = B.cg_solve_multi(op, m, Bk, X0)
    check_against_oracle(O, rp, ci, va, -1, Bk, X0, X, hists, stats)
    op.free()


def test_cg_multi_max_iters_some_columns_converge(B, O, fresh_host_matrices):
    """max_iters = 5: the eigenmode columns converge (and are frozen), the others report like
    test_cg_not_converged_reports_like_reference: 5 iterations, not converged, residual_norm = ||r0||."""
    n = 200
    N = n * n
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(9)
    Bk = np.stack([eigenmode(n), np.ones(N), rng.standard_normal(N), 3.0 * eigenmode(n)])
    X0 = np.zeros((4, N))
    X, hists, stats = B.cg_solve_multi(op, m, Bk, X0, max_iters=5)
    rp, ci, va = O.stencil5_csr(n)
    check_against_oracle(O, rp, ci, va, n, Bk, X0, X, hists, stats, max_iters=5)
    assert [s.converged for s in stats] == [1, 0, 0, 1] and [s.iterations for s in stats] == [1, 5, 5, 1]
    for j in (1, 2):
        assert stats[j].residual_norm == hists[j][0] and len(hists[j]) == 6
    assert stats[1].residual_norm == float(n)  # ||1|| = n exactly
    op.free()


def stats_tuple(s):
    return (s.iterations, s.residual_norm, s.converged, s.solution_sum, s.solution_norm)


def printed(capfd):
    """What the library's printf calls wrote since the last call, as lines (C's stdout is flushed first: it is not a terminal here)."""
    ctypes.CDLL(None).fflush(None)
    return capfd.readouterr().out.splitlines()


def expected_print_out(tag, hists, stats, verbose, initial_suffix="", breakdown=()):
    """The whole print-out of a batched solve at `verbose`, from what the solve returned: the initial residuals, under verbose 2
    one Iter line per iteration and column that took part in it, each column's verdict, then the time breakdown."""
    k = len(hists)
    lines = ["[%s %d] Initial residual: %e%s" % (tag, j, hists[j][0], initial_suffix) for j in range(k)]
    if verbose >= 2:
        for it in range(1, max(s.iterations for s in stats) + 1):
            for j in range(k):
                if it <= stats[j].iterations:
                    rel = hists[j][it] / hists[j][0] if hists[j][0] != 0.0 else float("nan")
                    lines.append("[%s %d] Iter %3d: residual = %e (rel = %e)" % (tag, j, it, hists[j][it], rel))
    for j in range(k):
        if j in breakdown:
            lines.append("[%s %d] Breakdown in iteration %d (pAp or r.z zero or not finite)" % (tag, j, stats[j].iterations))
        lines += ["[%s %d] Converged: %s" % (tag, j, "YES" if stats[j].converged else "NO"),
                  "[%s %d] Iterations: %d" % (tag, j, stats[j].iterations),
                  "[%s %d] Final residual: %e" % (tag, j, stats[j].residual_norm)]
    t = stats[0]
    return lines + ["[%s] %d systems, time breakdown (whole batch):" % (tag, k), "     Total:      %.3f ms" % t.time_total_ms,
                    "     SpMV:       %.3f ms" % t.time_spmv_ms, "     BLAS1:      %.3f ms" % t.time_blas1_ms,
                    "     Reductions: %.3f ms" % t.time_reductions_ms]


def check_print_out(got, want):
    """Line for line; 0 / 0 of a zero column prints as nan or -nan."""
    assert [g.replace("-nan", "nan") for g in got] == want, "\n".join(got)


def check_verbose_changes_nothing_else(silent, loud, verbose):
    """x and the histories bit for bit; the statistics too, but for residual_norm of a column that did not converge, which is the
    last residual under verbose 2 and ||r0|| else (the reference's rule, solve_common.hpp)."""
    for j in range(len(silent[1])):
        assert np.array_equal(loud[0][j], silent[0][j]) and np.array_equal(loud[1][j], silent[1][j]), j
        if verbose < 2 or silent[2][j].converged or silent[2][j].iterations == 0:
            assert stats_tuple(loud[2][j]) == stats_tuple(silent[2][j]), j
        else:
            assert stats_tuple(loud[2][j])[:1] + stats_tuple(loud[2][j])[2:] == stats_tuple(silent[2][j])[:1] + stats_tuple(silent[2][j])[2:], j
            assert silent[2][j].residual_norm == silent[1][j][0] and loud[2][j].residual_norm == loud[1][j][-1], j


def test_cg_multi_print_out_and_late_refusals(B, O, fresh_host_matrices, capfd):
    """A 32 x 32 system with k = 3 (odd k: 8-byte accesses): the whole print-out of a solve under verbose 1, and under verbose 2
    with max_iters = 5 (the eigenmode column takes part in one iteration, the others in five), line for line; printing changes no
    bit of what the solve returns. Then max_iters < 0 on an initialised operator, and the refusal only such an operator reaches: a
    system that is not of the operator's size."""
    n = 32
    N = n * n
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    Bk = np.stack([np.ones(N), np.random.default_rng(32).standard_normal(N), eigenmode(n)])
    X0 = np.zeros((3, N))
    for verbose, kw in ((1, {}), (2, {"max_iters": 5})):
        silent = B.cg_solve_multi(op, m, Bk, X0, **kw)
        printed(capfd)
        loud = B.cg_solve_multi(op, m, Bk, X0, verbose=verbose, **kw)
        got = printed(capfd)
        check_verbose_changes_nothing_else(silent, loud, verbose)
        check_print_out(got, expected_print_out("CG-MULTI", loud[1], loud[2], verbose))
        assert len([l for l in got if " Iter " in l]) == (0 if verbose == 1 else 5 + 5 + 1)
        assert [s.converged for s in loud[2]] == ([1, 1, 1] if verbose == 1 else [0, 0, 1])
    L = B._multi_lib()
    stats = (B.CGStats * 3)()
    X = X0.copy()
    cfg = B.CGConfig(-1, 1e-6, 0, 0)
    capfd.readouterr()
    assert L.spmv_amd_cg_solve_device_multi(op.op, m.ptr, 3, Bk.ctypes.data, X.ctypes.data, ctypes.byref(cfg), stats) != 0
    assert "[CG-MULTI] max_iters < 0" in capfd.readouterr().err
    small = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N - 1, N - 1, -1)
    with pytest.raises(RuntimeError):
        B.cg_solve_multi(op, small, Bk, X0)
    err = capfd.readouterr().err
    assert "[CG-MULTI] the operator holds a %d x %d matrix, mat->rows = %d: a square system of that size is required" % (N, N, N - 1) in err
    op.free()


@pytest.mark.parametrize("n, mode", [(200, "stencil5-csr"), (512, "stencil5-csr"), (200, "cusparse-csr")])
def test_cg_multi_columns_are_independent_bit_for_bit(B, O, fresh_host_matrices, n, mode):
    """n = 200 takes row-direct, n = 512 row-lds, cusparse-csr the flat-row kernel: each has its own dot-partial geometry."""
    N = n * n
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    op = B.Operator(mode)
    assert op.init(m) == 0
    assert op.spmm_variant() == {(200, "stencil5-csr"): "spmm/stencil5-row-direct", (512, "stencil5-csr"): "spmm/stencil5-row-lds",
                                 (200, "cusparse-csr"): "spmm/csr"}[(n, mode)]
    rng = np.random.default_rng(11)
    base = rng.standard_normal(N)
    Bk = np.stack([base, np.ones(N), eigenmode(n), rng.standard_normal(N), 2.0 * base, np.ones(N) + 0.01 * np.sin(np.arange(N)),
                   rng.uniform(0, 1, N), 0.5 * np.ones(N)])
    X, hists, stats = B.cg_solve_multi(op, m, Bk, np.zeros_like(Bk))
    # permuted columns: every column's history, x and statistics bit-identical
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    Xp, hp, sp = B.cg_solve_multi(op, m, Bk[perm], np.zeros_like(Bk))
    for slot, j in enumerate(perm):
        assert np.array_equal(Xp[slot], X[j]) and np.array_equal(hp[slot], hists[j]), (slot, j)
        assert stats_tuple(sp[slot]) == stats_tuple(stats[j])
    # the same column alone, in pairs, in threes, ... in eights
    for k in KS:
        cols = [(3 + i) % 8 for i in range(k)]
        Xk, hk, sk = B.cg_solve_multi(op, m, Bk[cols], np.zeros((k, N)))
        for slot, j in enumerate(cols):
            assert np.array_equal(Xk[slot], X[j]) and np.array_equal(hk[slot], hists[j]), (k, slot, j)
            assert stats_tuple(sk[slot]) == stats_tuple(stats[j])
    # b and 2b: scaling by 2 is exact, so the histories and solutions are exactly doubled
    assert np.array_equal(hists[4], 2.0 * hists[0]) and np.array_equal(X[4], 2.0 * X[0])
    assert stats[4].iterations == stats[0].iterations
    op.free()


@pytest.mark.parametrize("n", [130, 512])
def test_cg_multi_a_bad_column_leaves_its_neighbours_alone(B, O, fresh_host_matrices, n):
    """One column whose right-hand side is zero (0 / 0 in the first alpha) or holds one NaN, in slot 0, slot 1 or the last slot of
    a batch of 2, 5 or 6 (pairs of columns share 16-byte loads and stores where k is even): every healthy column's x, history and
    statistics are bit for bit those of the batch without the bad column; the bad column never meets the stopping test, as in
    the oracle: max_iters iterations, not converged, a history of max_iters + 1 entries. The call returns 0."""
    N = n * n
    iters = 8
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    rp, ci, va = O.stencil5_csr(n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(17)
    healthy = np.stack([rng.standard_normal(N), eigenmode(n), np.ones(N), rng.uniform(0, 1, N), np.ones(N) + 0.01 * np.sin(np.arange(N))])
    one_nan = rng.standard_normal(N)
    one_nan[N // 2 + 1] = np.nan
    for what, bad in (("zero", np.zeros(N)), ("nan", one_nan)):
        _, ho, ro = O.cg(rp, ci, va, n, bad, np.zeros(N), max_iters=iters)
        assert ro.iterations == iters and not ro.converged and len(ho) == iters + 1
        for k in (2, 5, 6):
            Xh, hh, sh = B.cg_solve_multi(op, m, healthy[:k - 1], np.zeros((k - 1, N)), max_iters=iters)  # raises unless it returns 0
            assert k == 2 or sh[1].converged == 1  # the eigenmode: a frozen column next to the bad one
            for slot in sorted({0, 1, k - 1}):
                Bk = np.insert(healthy[:k - 1], slot, bad, axis=0)
                X, hists, stats = B.cg_solve_multi(op, m, Bk, np.zeros((k, N)), max_iters=iters)
                assert stats[slot].iterations == ro.iterations and stats[slot].converged == ro.converged, (what, k, slot)
                assert len(hists[slot]) == len(ho), (what, k, slot)
                others = [s for s in range(k) if s != slot]
                for j, s in enumerate(others):
                    assert np.array_equal(X[s], Xh[j]) and np.array_equal(hists[s], hh[j]), (what, k, slot, s)
                    assert stats_tuple(stats[s]) == stats_tuple(sh[j]), (what, k, slot, s)
                    assert np.all(np.isfinite(X[s])) and np.all(np.isfinite(hists[s])), (what, k, slot, s)
    op.free()


def test_cg_multi_coexists_with_cg_solve_device(B, O, fresh_host_matrices):
    n = 512
    N = n * n
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(13)
    b = rng.standard_normal(N)
    x1, h1, s1 = B.cg_solve(op, m, b, np.zeros(N), device=True)
    Bk = np.stack([b, np.ones(N), eigenmode(n), 2.0 * b])
    X, hists, stats = B.cg_solve_multi(op, m, Bk, np.zeros((4, N)))
    x2, h2, s2 = B.cg_solve(op, m, b, np.zeros(N), device=True)
    assert np.array_equal(x1, x2) and np.array_equal(h1, h2) and stats_tuple(s1) == stats_tuple(s2)
    # refusals leave the operator usable
    ell = B.Operator("ellpack")
    with pytest.raises(RuntimeError):
        B.cg_solve_multi(ell, m, Bk, np.zeros((4, N)))
    with pytest.raises(RuntimeError):
        B.cg_solve_multi(op, m, np.ones((9, N)), np.zeros((9, N)))
    assert B._multi_lib().spmv_amd_spmm_device(b"stencil5-csr", 9, None, None) != 0
    X2, hists2, stats2 = B.cg_solve_multi(op, m, Bk, np.zeros((4, N)))
    assert np.array_equal(X2, X) and all(np.array_equal(a, c) for a, c in zip(hists2, hists))
    x3, h3, s3 = B.cg_solve(op, m, b, np.zeros(N), device=True)
    assert np.array_equal(x3, x1) and np.array_equal(h3, h1)
    op.free()


def test_operator_free_and_release_workspace_release_the_multi_workspace(B, O, fresh_host_matrices):
    """The batched workspace (four block vectors) is held between solves and released by an operator's free() and by
    spmv_amd_cg_release_workspace(), as cg_solve_device's is; the library's own count, not the device's free memory (which
    other processes on the GPU move)."""
    n = 1024
    N = n * n
    vectors = 4 * N * 8 * 8  # four block vectors of 8 columns: 268 MB
    m = B.HostMatrix(O.stencil5_coo(n), N, N, n)
    L = B._multi_lib()
    for release in ("free", "release_workspace"):
        op = B.Operator("stencil5-csr")
        assert op.init(m) == 0
        X, hists, stats = B.cg_solve_multi(op, m, np.ones((8, N)), np.zeros((8, N)), max_iters=3)
        held = L.spmv_amd_cg_multi_workspace_bytes()
        assert vectors <= held < 1.1 * vectors, held
        if release == "free":
            op.free()
            assert L.spmv_amd_cg_multi_workspace_bytes() == 0
        else:
            B.lib().spmv_amd_cg_release_workspace()
            assert L.spmv_amd_cg_multi_workspace_bytes() == 0
            # and the operator still solves (a fresh workspace)
            X2, h2, s2 = B.cg_solve_multi(op, m, np.ones((8, N)), np.zeros((8, N)), max_iters=3)
            assert np.array_equal(X2, X) and L.spmv_amd_cg_multi_workspace_bytes() == held
            op.free()
            assert L.spmv_amd_cg_multi_workspace_bytes() == 0


@pytest.mark.parametrize("mode", ["stencil5-csr", "cusparse-csr"])
def test_spmm_on_8_byte_aligned_block_vectors(B, O, fresh_host_matrices, mode):
    """X / Y one double into their allocations (8- but not 16-byte aligned): even k takes the 8-byte-access kernels, still
    bit for bit; the doubles around Y are not touched."""
    n = 700
    rows = n * n
    e = random_stencil(O, n, 31)
    rp, ci, va = O.build_csr(e, rows)
    m = B.HostMatrix(e, rows, rows, n)
    X = np.random.default_rng(31).standard_normal((8, rows))
    op = B.Operator(mode)
    assert op.init(m) == 0
    L = B._multi_lib()
    for forced in (("row-lds", "row-direct", "row-generic") if mode == "stencil5-csr" else (None,)):
        op.select_variant(forced)
        for k in KS:
            inter = np.ascontiguousarray(X[:k].T).ravel()  # interleaved: [row * k + j]
            dx = B.DeviceVector.from_host(np.concatenate([[0.0], inter]))
            dy = B.DeviceVector(rows * k + 2, fill=-7.0)
            assert L.spmv_amd_spmm_device(mode.encode(), k, dx.ptr + 8, dy.ptr + 8) == 0
            got = dy.to_host()
            dx.free(), dy.free()
            assert got[0] == -7.0 and got[-1] == -7.0
            Y = got[1:-1].reshape(rows, k).T
            for j in range(k):
                want = O.spmv_stencil5(rp, ci, va, X[j], n) if mode == "stencil5-csr" else O.spmv_csr(rp, ci, va, X[j])
                assert np.array_equal(Y[j], want), (forced, k, j)
    op.select_variant(None)
    op.free()
