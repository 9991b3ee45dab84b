"""Jacobi-preconditioned CG (spmv_amd_pcg_solve_device, csrc/pcg.hip) on the GPU: the value it adds on a matrix whose diagonal
varies, bit-exact inverse diagonals from all four operators, the golden anchors with kinds none / jacobi, refusals, breakdown,
coexistence with the other CG entry points, the Matrix Market path and the application's --precond; then the solves away from
x0 = 0: non-zero first guesses on odd, negative-definite and two-stage-reduction systems against the restatement AND the true
residual in long double, tiny systems, the stopping rules and statistics, the detailed timers, non-finite and zero right-hand
sides, and the workspace across sizes and operators (tests/test_pcg_stages_gpu.py has the kernels one by one)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import conftest
from conftest import GOLDEN, ROOT
from pcg_restatement import TABLE, diagonal, entries_of, hist_err, pcg, scaled_stencil5, stencil5, table_system, true_residual_norm

pytestmark = pytest.mark.gpu
TOL = 1e-10
OPERATORS = ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack")


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_reset_host_matrices()


def _close(x, want):
    return np.max(np.abs(x - want)) <= TOL * np.max(np.abs(want))


def test_jacobi_converges_where_cg_does_not(B):
    """S A S, s_i = 10^U(0, 2), 128^2, seed 1: cg_solve_device does not converge in 200 iterations, Jacobi-PCG converges in the
    restatement's 24 with its history and x (tests/test_pcg_host.py pins the restatement against scipy)."""
    n = 128
    A = scaled_stencil5(n, 2, 1)
    rows = n * n
    b = np.ones(rows)
    xo, ho, ito, conv = pcg(A, b, np.zeros(rows), 1.0 / diagonal(A), 1e-6, 200)
    assert conv and ito == 24
    m = B.HostMatrix(entries_of(A), rows, rows, n)
    for mode in ("cusparse-csr", "stencil5-csr"):
        B.lib().spmv_amd_reset_host_matrices()
        op = B.Operator(mode)
        assert op.init(m) == 0
        _, _, st = B.cg_solve(op, m, b, np.zeros(rows), max_iters=200)
        assert st.converged == 0 and st.iterations == 200, mode
        pc = B.Precond(op, "jacobi")
        assert pc.kind == "jacobi"
        x, h, st = B.pcg_solve_device(op, m, pc, b, np.zeros(rows), max_iters=200)
        assert st.converged == 1 and st.iterations == ito, (mode, st.iterations)
        assert len(h) == ito + 1 and hist_err(h, ho) < TOL and _close(x, xo), mode
        assert st.residual_norm == h[-1] and abs(st.solution_sum - np.sum(x)) <= 1e-9 * abs(np.sum(x))
        pc.destroy()
        op.free()


def _general_spd_with_duplicate_diagonals(n, seed):
    """A random sparse SPD matrix whose diagonal entries arrive as two COO entries each (build_csr_struct keeps both, in input
    order); returns the entries and d as the library must compute it: (0.0 + first) + second."""
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=0.01, random_state=seed, data_rvs=lambda k: rng.uniform(-1.0, 1.0, k))
    A = sp.coo_matrix(sp.triu(R, 1) + sp.triu(R, 1).T)
    off = np.asarray(abs(sp.csr_matrix(A)).sum(axis=1)).ravel()
    first = off + rng.uniform(0.5, 4.0, n)
    second = rng.uniform(1e-3, 1.0, n) * np.pi
    e = np.zeros(A.nnz + 2 * n, dtype=entries_of(A).dtype)
    e[: A.nnz]["row"], e[: A.nnz]["col"], e[: A.nnz]["value"] = A.row, A.col, A.data
    idx = np.arange(n)
    e[A.nnz:A.nnz + n]["row"], e[A.nnz:A.nnz + n]["col"], e[A.nnz:A.nnz + n]["value"] = idx, idx, first
    e[A.nnz + n:]["row"], e[A.nnz + n:]["col"], e[A.nnz + n:]["value"] = idx, idx, second
    return e, (0.0 + first) + second


def test_inverse_diagonal_bits_are_the_same_from_every_operator(B, O):
    rng = np.random.default_rng(5)
    n = 96
    e = O.stencil5_coo(n)
    diag = e["row"] == e["col"]
    e["value"] = np.where(diag, rng.uniform(1.0, 10.0, len(e)), rng.uniform(-3.0, 3.0, len(e)))
    d_stencil = np.zeros(n * n)
    d_stencil[e["row"][diag]] = e["value"][diag]
    eg, d_general = _general_spd_with_duplicate_diagonals(3000, 9)
    for ents, rows, grid, d in ((e, n * n, n, d_stencil), (eg, 3000, -1, d_general)):
        want = 1.0 / d
        m = B.HostMatrix(ents, rows, rows, grid)
        for mode in OPERATORS:
            B.lib().spmv_amd_reset_host_matrices()
            op = B.Operator(mode)
            assert op.init(m) == 0, mode
            pc = B.Precond(op, "jacobi")
            got = pc.inverse_diagonal()
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (mode, grid)
            pc.destroy()
            op.free()
        pc = B.Precond.from_diagonal(d)
        assert np.array_equal(pc.inverse_diagonal().view(np.uint64), want.view(np.uint64))
        pc.destroy()


@pytest.mark.parametrize("case", ["81:5.0", "81:-4.0", "512:5.0", "2000:5.0"])
def test_golden_anchors_with_both_kinds(B, O, case):
    """The constant-diagonal stencil: Jacobi is a multiple of the identity, so both kinds reproduce the golden CG run
    (iterations, history within 1e-10). 81:-4.0 is negative definite: no sign test stands in the way."""
    gold = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["cases"][case]["cg"]
    n, center = int(case.split(":")[0]), float(case.split(":")[1])
    op = B.Operator("stencil5-csr")
    if center == 5.0 and n >= 512:
        assert op.init_synthetic(n) == 0
        m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n * n, n * n, n)
    else:
        m = B.HostMatrix(O.stencil5_coo(n, center, -1.0), n * n, n * n, n)
        assert op.init(m) == 0
    b = np.ones(n * n)
    for kind in ("none", "jacobi"):
        pc = B.Precond(op, kind)
        x, h, st = B.pcg_solve_device(op, m, pc, b, np.zeros(n * n))
        assert st.converged == 1 and st.iterations == gold["iterations"], (case, kind, st.iterations)
        assert hist_err(h, np.array(gold["history"])) < TOL, (case, kind)
        assert abs(st.solution_sum - gold["solution_sum"]) <= 1e-9 * abs(gold["solution_sum"])
        pc.destroy()
    op.free()


def _tridiagonal(n, diag):
    t = []
    for i in range(n):
        if diag[i] is not None:
            t.append((i, i, diag[i]))
        if i > 0:
            t.append((i, i - 1, -0.5))
        if i < n - 1:
            t.append((i, i + 1, -0.5))
    e = np.zeros(len(t), dtype=entries_of(sp.identity(1)).dtype)
    for k, v in enumerate(t):
        e[k] = v
    return e


def test_refusals_name_the_first_bad_row(B):
    n = 8
    cases = {3: [4.0, 4.0, 4.0, None, 4.0, 4.0, 4.0, 4.0], 2: [4.0, 4.0, 0.0, 4.0, 0.0, 4.0, 4.0, 4.0],
             4: [4.0, 4.0, 4.0, 4.0, np.nan, 4.0, np.inf, 4.0], 5: [4.0, 4.0, 4.0, 4.0, 4.0, -4.0, 4.0, 4.0],
             1: [-4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0]}
    for bad_row, diag in cases.items():
        for mode in ("cusparse-csr", "ellpack"):
            B.lib().spmv_amd_reset_host_matrices()
            op = B.Operator(mode)
            assert op.init(B.HostMatrix(_tridiagonal(n, diag), n, n, -1)) == 0
            with pytest.raises(ValueError) as err:
                B.Precond(op, "jacobi")
            assert err.value.bad_row == bad_row, (mode, diag)
            none = B.Precond(op, "none")  # kind none reads no diagonal
            assert none.kind == "none"
            none.destroy()
            op.free()
        d = np.array([0.0 if v is None else v for v in diag])
        with pytest.raises(ValueError) as err:
            B.Precond.from_diagonal(d)
        assert err.value.bad_row == bad_row


def test_stale_foreign_and_mismatched_preconditioners_are_refused(B):
    n = 32
    A = scaled_stencil5(n, 1, 4)
    rows = n * n
    m = B.HostMatrix(entries_of(A), rows, rows, n)
    b = np.ones(rows)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    pc, none = B.Precond(op, "jacobi"), B.Precond(op, "none")
    xo, ho, ito, _ = pcg(A, b, np.zeros(rows), 1.0 / diagonal(A))
    x1, h1, st = B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
    assert st.iterations == ito and hist_err(h1, ho) < TOL and _close(x1, xo)
    # another operator of this library, a caller's operator table, the wrong size
    ell = B.Operator("ellpack")
    assert ell.init(m) == 0
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(ell, m, pc, b, np.zeros(rows))
    ell.free()
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: op.op.contents.run_device(dx, dy))
    foreign = type("Foreign", (), {"op": C.pointer(own)})()
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(foreign, m, pc, b, np.zeros(rows))
    small = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows - 1, rows - 1, -1)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, small, pc, b, np.zeros(rows))
    # a caller's diagonal is the way in for a caller's operator
    pd = B.Precond.from_diagonal(diagonal(A))
    x, h, st = B.pcg_solve_device(foreign, m, pd, b, np.zeros(rows))
    assert st.iterations == ito and hist_err(h, ho) < TOL and _close(x, xo)
    # free() and a new init: both preconditioners belong to the old matrix
    op.free()
    assert op.init(m) == 0
    for stale in (pc, none):
        with pytest.raises(RuntimeError):
            B.pcg_solve_device(op, m, stale, b, np.zeros(rows))
    fresh = B.Precond(op, "jacobi")
    x2, h2, _ = B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
    assert np.array_equal(x2, x1) and np.array_equal(h2, h1)
    for p in (pc, none, pd, fresh):
        p.destroy()
    op.free()


def test_breakdown_stops_with_a_finite_x(B):
    """[[0, 1], [1, 0]], b = (1, 0), kind none: p.Ap = 0 in iteration 1 -- stop there, not converged, x untouched."""
    e = np.zeros(2, dtype=B.ENTRY_DTYPE)
    e[0], e[1] = (0, 1, 1.0), (1, 0, 1.0)
    m = B.HostMatrix(e, 2, 2, -1)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    x, h, st = B.pcg_solve_device(op, m, pc, np.array([1.0, 0.0]), np.zeros(2))
    assert st.iterations == 1 and st.converged == 0 and np.all(np.isfinite(x))
    assert len(h) == 2 and h[0] == 1.0
    with pytest.raises(ValueError):
        B.Precond(op, "jacobi")  # the diagonal is zero
    pc.destroy()
    op.free()


def test_coexistence_and_determinism(B):
    """PCG, cg_solve_device and the batched solver interleaved on one operator: each reproduces its own x and history bit for
    bit, a PCG solve leaves cg_solve_device's history alone, and free() releases the workspaces."""
    n = 64
    A = scaled_stencil5(n, 1, 2)
    rows = n * n
    m = B.HostMatrix(entries_of(A), rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(3)
    b = rng.standard_normal(rows)
    Bk = rng.standard_normal((2, rows))
    pc = B.Precond(op, "jacobi")
    runs = {"pcg": [], "cg": [], "multi": []}
    for _ in range(2):
        runs["pcg"].append(B.pcg_solve_device(op, m, pc, b, np.zeros(rows))[:2])
        runs["cg"].append(B.cg_solve(op, m, b, np.zeros(rows), max_iters=3000)[:2])
        B.pcg_solve_device(op, m, pc, Bk[0], np.zeros(rows))
        hc = np.zeros(3001)
        count = B.lib().spmv_amd_cg_last_history(hc.ctypes.data, len(hc))
        assert np.array_equal(hc[:count], runs["cg"][-1][1])  # untouched by the PCG solve
        X, H, _ = B.cg_solve_multi(op, m, Bk, np.zeros((2, rows)), max_iters=3000)
        runs["multi"].append((X, np.concatenate(H)))
    for name, (a, c) in runs.items():
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]), name
    xo, ho, ito, _ = pcg(A, b, np.zeros(rows), 1.0 / diagonal(A))
    assert len(runs["pcg"][0][1]) == ito + 1 and hist_err(runs["pcg"][0][1], ho) < TOL
    assert B._multi_lib().spmv_amd_cg_multi_workspace_bytes() > 0
    op.free()
    assert B._multi_lib().spmv_amd_cg_multi_workspace_bytes() == 0  # released with cg_solve_device's and the PCG workspace
    pc.destroy()


def test_matrix_market_general_path(B, tmp_path):
    """A variable-coefficient SPD matrix written as a SYMMETRIC Matrix Market file, read by load_matrix_market, solved through
    cusparse-csr and ellpack."""
    n = 48
    A = scaled_stencil5(n, 1, 6)
    L = sp.coo_matrix(sp.tril(A))
    path = tmp_path / "scaled.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{A.shape[0]} {A.shape[1]} {L.nnz}\n")
        for r, c, v in zip(L.row, L.col, L.data):
            f.write(f"{r + 1} {c + 1} {float(v)!r}\n")
    m = B.load_matrix_market(str(path))
    rows = n * n
    assert m.c.rows == rows
    b = np.ones(rows)
    xo, ho, ito, conv = pcg(A, b, np.zeros(rows), 1.0 / diagonal(A))
    assert conv
    for mode in ("cusparse-csr", "ellpack"):
        B.lib().spmv_amd_reset_host_matrices()
        op = B.Operator(mode)
        assert op.init(m) == 0
        pc = B.Precond(op, "jacobi")
        x, h, st = B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
        assert st.converged == 1 and st.iterations == ito and hist_err(h, ho) < TOL and _close(x, xo), mode
        pc.destroy()
        op.free()


def test_application_precond_flag(B):
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    gold = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["cases"]["512:5.0"]["cg"]
    out = subprocess.run([exe, "--stencil=512", "--precond=jacobi"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert f"--- Results for stencil5-csr+jacobi ---\nConverged: YES in {gold['iterations']} iterations" in out.stdout
    refused = subprocess.run([exe, "--stencil=64", "--precond=jacobi", "--host"], capture_output=True, text=True, timeout=60)
    assert refused.returncode != 0 and "--precond" in refused.stderr
    plain = subprocess.run([exe, "--stencil=512"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "Preconditioner" not in plain.stdout
    assert f"--- Results for stencil5-csr ---\nConverged: YES in {gold['iterations']} iterations" in plain.stdout


# ---------------------------------------------------------------- away from x0 = 0 (pcg_restatement.TABLE; tests/test_pcg_host.py
# holds every row of it in two roundings of the restatement)

@functools.lru_cache(maxsize=None)
def _system(name):
    A, b, x0 = table_system(name)
    return A, b, x0, entries_of(A)


@functools.lru_cache(maxsize=None)
def _restated(name, kind, tol, max_iters):
    """The restatement's x, history, iterations, verdict on a table system, and its own g (see _true_residual_gap)."""
    A, b, x0, e = _system(name)
    x, h, it, conv = pcg(A, b, x0, 1.0 / diagonal(A) if kind == "jacobi" else None, tol, max_iters)
    return x, h, it, conv, _true_residual_gap(e, b, x, h)


def _true_residual_gap(entries, b, x, h):
    """g = | ||b - A x|| - h[-1] | / h[-1], the true residual accumulated in long double from the COO entries."""
    return abs(true_residual_norm(entries, b, x) - h[-1]) / h[-1]


def _foreign(B, op):
    """A caller's own operator table around `op`'s device product (the library does not know its matrix)."""
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: op.op.contents.run_device(dx, dy))
    return type("Foreign", (), {"op": C.pointer(own), "_keep": own})()


@pytest.mark.parametrize("row", range(len(TABLE)), ids=[f"{r[0]}-{r[1]}-{r[2]:g}-{r[3]}" for r in TABLE])
def test_nonzero_first_guess_against_restatement_and_true_residual(B, row):
    """x0 = standard_normal on every system of the table: iterations equal to the restatement's, history within 1e-10
    (conftest.hist_err), x within 1e-10 -- `jacobi` through all four operators, `none` through a fused (stencil5-csr) and an unfused
    (ellpack) one, the 127^2 system also through a caller's operator table with a caller's diagonal. A converged solve is also
    held to something that shares no algebra with the restatement: g = | ||b - A x|| - h[-1] | / h[-1] in long double must be
    at most 100 x the restatement's own g on the same case (floor 1e-12): the factor covers another summation order, a lost x0
    or a wrong alpha in the x update misses it by ten orders of magnitude. x0 = 0 must give another h[0] (x0 is not ignored on
    both sides).
    Largest GPU g / restatement g seen on the MI355X: 6.3 (601^2 unscaled, jacobi, tol 1e-6, cusparse-csr: 1.5e-13 against
    2.3e-14); 55 of the 60 converged solves lie between 0.05 and 3.5."""
    name, kind, tol, max_iters, iterations = TABLE[row]
    A, b, x0, e = _system(name)
    xo, ho, ito, conv, g_ref = _restated(name, kind, tol, max_iters)
    assert ito == iterations and conv == (max_iters == 1000)
    rows, n = A.shape[0], int(round(np.sqrt(A.shape[0])))
    m = B.HostMatrix(e, rows, rows, n)
    for mode in OPERATORS if kind == "jacobi" else ("stencil5-csr", "ellpack"):
        B.lib().spmv_amd_reset_host_matrices()
        op = B.Operator(mode)
        assert op.init(m) == 0, mode
        solvers = [(mode, op, B.Precond(op, kind))]
        if name == "scaled127" and kind == "jacobi" and mode == "cusparse-csr":
            solvers.append(("caller's table", _foreign(B, op), B.Precond.from_diagonal(diagonal(A))))
        for label, who, pc in solvers:
            x, h, st = B.pcg_solve_device(who, m, pc, b, x0, max_iters=max_iters, tol=tol)
            case = (name, kind, tol, label)
            assert st.iterations == ito and st.converged == int(conv) and len(h) == ito + 1, (case, st.iterations)
            assert conftest.hist_err(h, ho) < TOL and _close(x, xo), (case, conftest.hist_err(h, ho))
            if conv:
                g = _true_residual_gap(e, b, x, h)
                print(f"{case}: g = {g:.3e}, the restatement's {g_ref:.3e}, ratio {g / g_ref:.3f}")
                assert g <= max(100.0 * g_ref, 1e-12), (case, g, g_ref)
            _, h0, _ = B.pcg_solve_device(who, m, pc, b, np.zeros(rows), max_iters=0, tol=tol)
            assert len(h0) == 1 and abs(h0[0] - h[0]) > 1e-3 * h[0], case
            pc.destroy()
        op.free()


def _dense_entries(B, M):
    M = np.atleast_2d(np.asarray(M, dtype=np.float64))
    t = [(i, j, M[i, j]) for i in range(M.shape[0]) for j in range(M.shape[1]) if M[i, j] != 0.0]
    e = np.zeros(len(t), dtype=B.ENTRY_DTYPE)
    for k, v in enumerate(t):
        e[k] = v
    return e


def test_tiny_systems_terminate_exactly(B):
    """1 x 1 ([[3]], b = 2, x0 = 0.5: one iteration, x = 2/3), 2 x 2 ([[4, 1], [1, 3]], b = (1, 2), x0 = (2, 1): two, x = (1/11,
    7/11)) and the 3 x 3 grid stencil from a random x0: the last residual is rounding noise, so x, the iteration count and the
    history through conftest.hist_err (noise against noise is not compared relatively)."""
    rng = np.random.default_rng(33)
    cases = [(np.array([[3.0]]), np.array([2.0]), np.array([0.5]), -1, 1, np.array([2.0 / 3.0]), ("cusparse-csr", "ellpack")),
             (np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([1.0, 2.0]), np.array([2.0, 1.0]), -1, 2, np.array([1.0 / 11.0, 7.0 / 11.0]),
              ("cusparse-csr", "ellpack")),
             (stencil5(3).toarray(), rng.standard_normal(9), rng.standard_normal(9), 3, None, None, ("cusparse-csr", "ellpack", "stencil5-csr"))]
    for M, b, x0, grid, iterations, exact, modes in cases:
        A = sp.csr_matrix(M)
        rows = A.shape[0]
        m = B.HostMatrix(_dense_entries(B, M), rows, rows, grid)
        for kind in ("none", "jacobi"):
            xo, ho, ito, conv = pcg(A, b, x0, 1.0 / diagonal(A) if kind == "jacobi" else None)
            assert conv and (iterations is None or ito == iterations), (rows, kind, ito)
            if exact is not None:
                assert _close(xo, exact)
            for mode in modes:
                B.lib().spmv_amd_reset_host_matrices()
                op = B.Operator(mode)
                assert op.init(m) == 0
                pc = B.Precond(op, kind)
                x, h, st = B.pcg_solve_device(op, m, pc, b, x0)
                case = (rows, kind, mode)
                assert st.converged == 1 and st.iterations == ito and len(h) == ito + 1, (case, st.iterations)
                assert _close(x, xo) and conftest.hist_err(h, ho) < TOL, case
                if exact is not None:
                    assert _close(x, exact), case
                pc.destroy()
                op.free()


def _jacobi_127(B, mode="stencil5-csr"):
    A, b, x0, e = _system("scaled127")
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(e, A.shape[0], A.shape[0], 127)
    op = B.Operator(mode)
    assert op.init(m) == 0
    return A, b, x0, m, op, B.Precond(op, "jacobi")


def test_stopping_rules_and_statistics(B, capfd):
    """max_iters = 0 and 5, a full solve after a capped one and a capped one after a full one (the history is the last solve's),
    residual_norm / converged by the reference's rule (fill_device_stats: ||r0|| unless the device converged or verbose >= 2), and
    tolerances other than 1e-6 -- on the 127^2 jacobi system of the table."""
    A, b, x0, m, op, pc = _jacobi_127(B)
    xo, ho, ito, _, _ = _restated("scaled127", "jacobi", 1e-6, 1000)
    x, h, st = B.pcg_solve_device(op, m, pc, b, x0, max_iters=0)
    assert st.iterations == 0 and st.converged == 0 and len(h) == 1 and np.array_equal(x, x0)
    assert abs(h[0] - ho[0]) <= TOL * ho[0] and st.residual_norm == h[0]
    x5, h5, st5 = B.pcg_solve_device(op, m, pc, b, x0, max_iters=5)
    assert st5.iterations == 5 and len(h5) == 6 and st5.converged == 0 and st5.residual_norm == h5[0]
    xf, hf, stf = B.pcg_solve_device(op, m, pc, b, x0)
    assert stf.iterations == ito and stf.converged == 1 and len(hf) == ito + 1 and stf.residual_norm == hf[-1]
    assert np.array_equal(h5, hf[:6])  # bit for bit
    assert conftest.hist_err(hf, ho) < TOL and _close(xf, xo)
    x5b, h5b, st5b = B.pcg_solve_device(op, m, pc, b, x0, max_iters=5, verbose=2)
    capfd.readouterr()  # the per-iteration lines
    assert len(h5b) == 6 and np.array_equal(h5b, h5) and np.array_equal(x5b, x5)  # not the earlier solve's 19 entries
    assert st5b.iterations == 5 and st5b.residual_norm == h5b[5] and st5b.converged == 0
    assert not _close(x5, xo)
    for tol in (1e-10, 1e-2):
        xt, ht, it, conv = pcg(A, b, x0, 1.0 / diagonal(A), tol)
        assert conv and (abs(ht[-1] / ht[0] / tol - 1.0) > 1e-6)
        x, h, st = B.pcg_solve_device(op, m, pc, b, x0, tol=tol)
        assert st.iterations == it and st.converged == 1 and len(h) == it + 1, (tol, st.iterations, it)
        assert conftest.hist_err(h, ht) < TOL and _close(x, xt) and st.residual_norm == h[-1], tol
        assert h[-1] / h[0] < tol <= h[-2] / h[0]
    pc.destroy()
    op.free()


def test_detailed_timers_change_no_bit(B):
    """enable_detailed_timers = 1 (events between the launches): x and history bit-identical to the plain solve, each of the
    three stage times > 0 and their sum <= the total; the plain solve reports the three as 0."""
    for mode in ("stencil5-csr", "ellpack"):  # fused p.Ap, and run_device + the dot pass
        _, b, x0, m, op, pc = _jacobi_127(B, mode)
        x, h, st = B.pcg_solve_device(op, m, pc, b, x0)
        xt, ht, stt = B.pcg_solve_device(op, m, pc, b, x0, timers=1)
        assert np.array_equal(xt, x) and np.array_equal(ht, h) and stt.iterations == st.iterations and stt.converged == 1, mode
        assert st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0
        assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0
        assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms, mode
        pc.destroy()
        op.free()


def test_non_finite_and_zero_right_hand_sides(B):
    """Ordinary values through the ordinary kernels: b with one inf (p.Ap is not finite) and b = 0 with x0 = 0 (p.Ap = 0): the first
    iteration breaks down -- return 0, converged = 0, iterations = 1, x bit-equal x0 (api.h: "stops the solve in that iteration
    with converged = 0 and x finite")."""
    for mode in ("stencil5-csr", "ellpack"):
        A, b, x0, m, op, _pc = _jacobi_127(B, mode)
        _pc.destroy()
        rows = A.shape[0]
        b_inf = b.copy()
        b_inf[rows // 2 + 3] = np.inf
        for kind in ("jacobi", "none"):
            pc = B.Precond(op, kind)
            for rhs, start in ((b_inf, x0), (b_inf, np.zeros(rows)), (np.zeros(rows), np.zeros(rows))):
                x, h, st = B.pcg_solve_device(op, m, pc, rhs, start)
                case = (mode, kind, float(rhs[rows // 2 + 3]))
                assert st.iterations == 1 and st.converged == 0 and len(h) == 2, (case, st.iterations, st.converged)
                assert np.array_equal(x, start) and np.all(np.isfinite(x)), case
            # the solver is as good as before afterwards
            x, h, st = B.pcg_solve_device(op, m, pc, b, x0, max_iters=5)
            assert st.iterations == 5 and np.all(np.isfinite(h)) and np.all(np.isfinite(x)), (mode, kind)
            pc.destroy()
        op.free()


def test_workspace_across_sizes_and_operators(B):
    """600^2 on stencil5-csr (fused p.Ap, 2813 partials), 127^2 on ellpack (dot pass) and 600^2 on stencil5-csr again in one
    process, no free() in between: the workspace is re-made at each change of size, the first and the third solve agree bit for
    bit, and the one in the middle is the restatement's."""
    A6, b6, x06, e6 = _system("scaled600")
    A1, b1, x01, e1 = _system("scaled127")
    B.lib().spmv_amd_reset_host_matrices()
    m6, m1 = B.HostMatrix(e6, A6.shape[0], A6.shape[0], 600), B.HostMatrix(e1, A1.shape[0], A1.shape[0], 127)
    big, small = B.Operator("stencil5-csr"), B.Operator("ellpack")
    assert big.init(m6) == 0 and small.init(m1) == 0
    pc6, pc1 = B.Precond(big, "jacobi"), B.Precond(small, "jacobi")
    first = B.pcg_solve_device(big, m6, pc6, b6, x06)
    middle = B.pcg_solve_device(small, m1, pc1, b1, x01)
    third = B.pcg_solve_device(big, m6, pc6, b6, x06)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2].iterations == third[2].iterations
    for (x, h, st), name in ((first, "scaled600"), (middle, "scaled127")):
        xo, ho, ito, _, _ = _restated(name, "jacobi", 1e-6, 1000)
        assert st.converged == 1 and st.iterations == ito and conftest.hist_err(h, ho) < TOL and _close(x, xo), name
    pc6.destroy(), pc1.destroy()
    big.free(), small.free()
