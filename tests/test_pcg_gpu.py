"""Jacobi-preconditioned CG (spmv_amd_pcg_solve_device, csrc/pcg.hip) on the GPU: the value it adds on a matrix whose diagonal
varies, bit-exact inverse diagonals from all four operators, the golden anchors with kinds none / jacobi, refusals, breakdown,
coexistence with the other CG entry points, the Matrix Market path and the application's --precond."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, ROOT
from pcg_restatement import diagonal, entries_of, hist_err, pcg, scaled_stencil5

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
