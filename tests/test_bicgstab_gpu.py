"""BiCGSTAB (spmv_amd_bicgstab_solve_device, csrc/bicgstab.hip) on the GPU: whole solves of the nonsymmetric table systems, BIT for
bit against bicgstab_restatement.bicgstab_exact -- the operator's own product, the dots as the kernels sum them, every update an
fma -- and within the row's third-rounding bound of plain numpy; every operator and variant against the exact form built on ITS
product; the 3-D twin; the breakdowns and the half step on 2 x 2 systems; agreement with PCG on a symmetric definite matrix;
determinism, max_iters = 0, the workspace's life, refusals that need a device, and the application's --solver
(tests/test_bicgstab_stages_gpu.py has the kernels one by one, tests/test_bicgstab_host.py the soundness of the inputs)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from bicgstab_restatement import (APP_CASE, TABLE, bicgstab, bicgstab_exact, convdiff5, dinv_of, entries_of, hist_err, table_system,
                                  third_rounding_bound)
from conftest import GOLDEN, ROOT
from pcg_restatement import stencil5

pytestmark = pytest.mark.gpu
ROWLDS_KNOB = "SPMV_AMD_ROWLDS_MIN_GRID"
# the table rows solved on stencil5-csr: every 2-D grid up to 127 (row-direct, and row-lds forced by the knob), one 600 and one 601
# row (row-lds by itself; 2813 and 2822 partials: the two-stage reduction; the 601 row ends by the half step)
SMALL = [i for i, r in enumerate(TABLE) if r[0] in ("grid33", "grid65", "grid127", "rows127")]
LARGE = [i for i, r in enumerate(TABLE) if (r[0], r[1], r[2]) in (("rows600", "jacobi", 1e-6), ("grid601", "none", 1e-10))]
CUBE = [i for i, r in enumerate(TABLE) if r[0] == "cube16"]


def row_id(i):
    return f"{TABLE[i][0]}-{TABLE[i][1]}-{TABLE[i][2]:g}"


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_reset_host_matrices()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def _csr(name):
    from oracle import oracle as O

    A, _, _ = table_system(name)
    e = entries_of(A)
    return (e,) + tuple(O.build_csr(e, A.shape[0]))


@functools.lru_cache(maxsize=None)
def _exact(name, kind, tol, family, max_iters=1000):
    """bicgstab_exact on a table system with the product of one operator family: "stencil5" (oracle.spmv_stencil5: stencil5-csr in
    all its variants, stencil5-ellpack) or "csr" (oracle.spmv_csr: the sequential CSR kernels, ellpack, stencil7-csr). Computed
    once, shared by every test that needs it."""
    from oracle import oracle as O

    A, b, x0 = table_system(name)
    _, rp, ci, va = _csr(name)
    grid = int(round(np.sqrt(A.shape[0])))
    matvec = (lambda u: O.spmv_stencil5(rp, ci, va, u, grid)) if family == "stencil5" else (lambda u: O.spmv_csr(rp, ci, va, u))
    return bicgstab_exact(matvec, b, x0, dinv_of(A, kind), tol, max_iters)


@functools.lru_cache(maxsize=None)
def _plain(name, kind, tol):
    A, b, x0 = table_system(name)
    return bicgstab(A, b, x0, dinv_of(A, kind), tol)


def check_exact(got, want, what):
    """(x, history, stats) of the device against (x, history, iterations, converged, end) of the exact form, bit for bit"""
    x, h, st = got
    wx, wh, wit, wconv, _ = want
    assert (st.iterations, st.converged) == (wit, int(wconv)) and len(h) == len(wh), (what, st.iterations, st.converged, wit, wconv)
    diff = np.flatnonzero(np.ascontiguousarray(h).view(np.uint64) != np.ascontiguousarray(wh).view(np.uint64))
    assert len(diff) == 0, (what, "history differs first at", int(diff[0]), float(h[diff[0]]), float(wh[diff[0]]))
    assert same_bits(x, wx), (what, float(np.max(np.abs(x - wx))))


def solve_row(B, row, mode, variant=None, expect_variant=None):
    name, kind, tol, _, _, _ = TABLE[row]
    A, b, x0 = table_system(name)
    dim = 3 if name.startswith("cube") else 2
    grid = int(round(A.shape[0] ** (1.0 / dim)))
    m = B.HostMatrix(_csr(name)[0], A.shape[0], A.shape[0], grid)
    op = B.Operator(mode)
    if variant is not None and mode != "stencil5-csr":  # the CSR operator's variant is chosen at init, the stencil operator's after it
        assert op.select_variant(variant) == 0
    try:
        assert op.init(m) == 0, mode
        if variant is not None and mode == "stencil5-csr":
            assert op.select_variant(variant) == 0
        if expect_variant is not None:
            assert op.variant() == expect_variant, op.variant()
        pc = B.Precond(op, kind)
        try:
            return B.bicgstab_solve(op, m, pc, b, x0, tol=tol)
        finally:
            pc.destroy()
    finally:
        op.free()
        if variant is not None:
            op.select_variant(None)


def check_row(B, row, got, family, what):
    name, kind, tol, iterations, end, stored = TABLE[row]
    want = _exact(name, kind, tol, family)
    assert want[2] == iterations and want[3] and want[4] == end, (what, want[2:])
    check_exact(got, want, what)
    x, h, st = got
    xp, hp, _, _, _ = _plain(name, kind, tol)
    bound = third_rounding_bound(stored)
    err = hist_err(h, hp)
    print(f"{what}: {st.iterations} iterations, ends by the {end} step, device against plain numpy {err:.2e} (bound {bound:.0e})")
    assert err <= bound and np.max(np.abs(x - xp)) <= bound * np.max(np.abs(xp)), (what, err)
    assert st.residual_norm == h[-1] and h[-1] / h[0] < tol <= h[-2] / h[0]


@pytest.mark.parametrize("form", ["row-direct", "row-lds"])
@pytest.mark.parametrize("row", SMALL, ids=row_id)
def test_table_rows_on_stencil5_csr_bit_for_bit(B, monkeypatch, row, form):
    if form == "row-lds":
        monkeypatch.setenv(ROWLDS_KNOB, "8")
    check_row(B, row, solve_row(B, row, "stencil5-csr", expect_variant="stencil5/" + form), "stencil5", (row_id(row), form))


@pytest.mark.parametrize("row", LARGE, ids=row_id)
def test_large_rows_on_row_lds_bit_for_bit(B, row):
    check_row(B, row, solve_row(B, row, "stencil5-csr", expect_variant="stencil5/row-lds"), "stencil5", row_id(row))


OTHERS = [("stencil5-csr", "row-generic", "stencil5/row-generic", "stencil5"), ("stencil5-ellpack", None, "ell/stencil5-direct", "stencil5"),
          ("cusparse-csr", "stream", "csr/stream", "csr"), ("cusparse-csr", "row-scalar", "csr/row-scalar", "csr"),
          ("ellpack", None, "ell/slot-major", "csr")]


@pytest.mark.parametrize("mode,variant,variant_name,family", OTHERS, ids=[o[2] for o in OTHERS])
@pytest.mark.parametrize("row", [i for i in SMALL if TABLE[i][0] in ("grid33", "grid65") and TABLE[i][2] == 1e-6], ids=row_id)
def test_every_operator_gives_the_bits_of_its_own_product(B, row, mode, variant, variant_name, family):
    """Every dot product of the solve is a streaming sum, whatever the operator: the only thing an operator contributes is the bits
    of A p. So stencil5/row-generic and stencil5-ellpack (the fma chain W, C, E, N, S: oracle.spmv_stencil5) give the bits of
    stencil5-csr's other variants, and the sequential CSR kernels and ellpack (the row in storage order: oracle.spmv_csr) give the
    bits of the exact form on THAT product. The two families round an interior row differently, so their solves are two roundings
    of one algebra: they agree within the row's third-rounding bound, not bit for bit (the figure is printed)."""
    got = solve_row(B, row, mode, variant, variant_name)
    check_row(B, row, got, family, (row_id(row), variant_name))
    name, kind, tol, _, _, stored = TABLE[row]
    other = _exact(name, kind, tol, "csr" if family == "stencil5" else "stencil5")
    across = hist_err(got[1], other[1])
    print(f"{row_id(row)} {variant_name}: against the other family's product {across:.2e}")
    assert across <= third_rounding_bound(stored)


@pytest.mark.parametrize("row", CUBE, ids=row_id)
def test_stencil7_csr_on_the_3d_twin(B, row):
    check_row(B, row, solve_row(B, row, "stencil7-csr"), "csr", row_id(row))


def _dense(B, M):
    M = np.atleast_2d(np.asarray(M, dtype=np.float64))
    t = [(i, j, M[i, j]) for i in range(M.shape[0]) for j in range(M.shape[1]) if M[i, j] != 0.0]
    e = np.zeros(len(t), dtype=B.ENTRY_DTYPE)
    for k, v in enumerate(t):
        e[k] = v
    return e


def _tiny(B, M, b, tol, max_iters=1000):
    from oracle import oracle as O

    n = len(b)
    e = _dense(B, M)
    B.lib().spmv_amd_reset_host_matrices()  # the systems share (rows, nnz)
    m = B.HostMatrix(e, n, n, -1)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, "none")
    got = B.bicgstab_solve(op, m, pc, b, np.zeros(n), tol=tol, max_iters=max_iters)
    pc.destroy()
    op.free()
    rp, ci, va = O.build_csr(e, n)
    want = bicgstab_exact(lambda u: O.spmv_csr(rp, ci, va, u), b, np.zeros(n), None, tol, max_iters)
    check_exact(got, want, (M, tol))
    return got + (want[4],)


def test_breakdowns_and_the_half_step_on_2x2_systems(B):
    """[[0, 1], [1, 0]], b = (1, 0): sigma = 0, iteration 1 breaks down, x stays 0, the history is [1, 1], converged = 0.
    3 I at tol 1e-6: the half step converges in iteration 1 with x = b / 3 exactly and no omega.
    The omega breakdown (t.t = 0) needs s = fma(-alpha, v, r) to be exactly 0, i.e. alpha exact: on 3 I alpha = fl(1 / 3) and the
    fma the algebra prescribes leaves s = b * 2^-54, not 0 (plain numpy, which rounds alpha * v first, does get 0 there:
    tests/test_bicgstab_host.py), so t.t is an ordinary number and the solve goes on -- held here to the exact form bit for bit.
    On 2 I alpha = 0.5 is exact: tol 0 gives the omega breakdown in iteration 1 with x = b / 2, the recorded residual 0 and
    converged = 0."""
    x, h, st, end = _tiny(B, [[0.0, 1.0], [1.0, 0.0]], np.array([1.0, 0.0]), 1e-6)
    assert end == "sigma" and st.iterations == 1 and st.converged == 0 and same_bits(x, [0.0, 0.0]) and same_bits(h, [1.0, 1.0])
    b = np.array([1.5, -0.75])
    x, h, st, end = _tiny(B, 3.0 * np.eye(2), b, 1e-6)
    assert end == "half" and st.iterations == 1 and st.converged == 1 and same_bits(x, b / 3.0) and len(h) == 2 and h[1] < 1e-15 * h[0]
    x, h, st, end = _tiny(B, 3.0 * np.eye(2), b, 0.0, max_iters=4)
    assert st.converged == 0 and np.all(np.isfinite(x)) and np.max(np.abs(x - b / 3.0)) <= 1e-15
    x, h, st, end = _tiny(B, 2.0 * np.eye(2), b, 0.0)
    assert end == "omega" and st.iterations == 1 and st.converged == 0 and same_bits(x, b / 2.0) and len(h) == 2 and h[1] == 0.0
    assert st.residual_norm == h[0]  # fill_device_stats: an unconverged solve without verbose reports ||r0||


def test_agrees_with_pcg_on_a_symmetric_definite_matrix(B):
    n = 127
    A = stencil5(n)
    rows = n * n
    rng = np.random.default_rng(n)
    b, x0 = rng.standard_normal(rows), rng.standard_normal(rows)
    m = B.HostMatrix(entries_of(A), rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    for kind in ("none", "jacobi"):
        pc = B.Precond(op, kind)
        xp, _, sp_ = B.pcg_solve_device(op, m, pc, b, x0, tol=1e-12)
        xb, _, sb = B.bicgstab_solve(op, m, pc, b, x0, tol=1e-12)
        assert sp_.converged == 1 and sb.converged == 1
        assert np.max(np.abs(xb - xp)) <= 1e-8 * np.max(np.abs(xp)), kind
        pc.destroy()
    op.free()


def test_determinism_max_iters_zero_statistics_and_the_workspace(B, capfd):
    """A solve run twice is bit-identical (with the detailed timers too, and after a solve of another size in between);
    max_iters = 0 returns x0 and a history of one entry; a capped solve's history is the full one's beginning; verbose 2 reports
    the last residual; PCG's history is left alone; a caller's operator table and a stale preconditioner."""
    row = next(i for i in SMALL if TABLE[i][:3] == ("rows127", "jacobi", 1e-6))
    name, kind, tol, iterations, _, _ = TABLE[row]
    A, b, x0 = table_system(name)
    rows = A.shape[0]
    m = B.HostMatrix(_csr(name)[0], rows, rows, 127)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    pc = B.Precond(op, kind)
    first = B.bicgstab_solve(op, m, pc, b, x0, tol=tol)
    _, hp, _ = B.pcg_solve_device(op, m, pc, b, x0)
    again = B.bicgstab_solve(op, m, pc, b, x0, tol=tol)
    timed = B.bicgstab_solve(op, m, pc, b, x0, tol=tol, timers=1)
    for other in (again, timed):
        assert same_bits(other[0], first[0]) and same_bits(other[1], first[1]) and other[2].iterations == iterations
    st, stt = first[2], timed[2]
    assert st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0
    assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0
    assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms
    assert abs(st.solution_sum - np.sum(first[0])) <= 1e-9 * np.sum(np.abs(first[0]))
    hp2 = np.zeros(len(hp) + 1)
    assert B._pcg_lib().spmv_amd_pcg_last_history(hp2.ctypes.data, len(hp2)) == len(hp) and same_bits(hp2[:len(hp)], hp)
    x, h, st0 = B.bicgstab_solve(op, m, pc, b, x0, tol=tol, max_iters=0)
    assert st0.iterations == 0 and st0.converged == 0 and len(h) == 1 and same_bits(x, x0) and same_bits(h, first[1][:1])
    x5, h5, st5 = B.bicgstab_solve(op, m, pc, b, x0, tol=tol, max_iters=5)
    assert st5.iterations == 5 and st5.converged == 0 and same_bits(h5, first[1][:6]) and st5.residual_norm == h5[0]
    capfd.readouterr()
    x5v, h5v, st5v = B.bicgstab_solve(op, m, pc, b, x0, tol=tol, max_iters=5, verbose=2)
    out = capfd.readouterr().out
    assert same_bits(x5v, x5) and same_bits(h5v, h5) and st5v.residual_norm == h5v[5]
    assert len(re.findall(r"\[BICGSTAB-DEVICE\] Iter +\d+: residual", out)) == 5 and "[BICGSTAB-DEVICE] Initial residual" in out and "[PCG" not in out
    # a caller's own operator table with a caller's diagonal: the same bits
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: op.op.contents.run_device(dx, dy))
    foreign = type("Foreign", (), {"op": C.pointer(own)})()
    pd = B.Precond.from_diagonal(np.asarray(A.diagonal()))
    theirs = B.bicgstab_solve(foreign, m, pd, b, x0, tol=tol)
    assert same_bits(theirs[0], first[0]) and same_bits(theirs[1], first[1])
    with pytest.raises(RuntimeError):
        B.bicgstab_solve(foreign, m, pc, b, x0)  # pc belongs to `op`
    pd.destroy()
    op.free()
    assert op.init(m) == 0
    with pytest.raises(RuntimeError):
        B.bicgstab_solve(op, m, pc, b, x0)  # made before the operator was last initialised
    fresh = B.Precond(op, kind)
    back = B.bicgstab_solve(op, m, fresh, b, x0, tol=tol)
    assert same_bits(back[0], first[0]) and same_bits(back[1], first[1])
    for p in (pc, fresh):
        p.destroy()
    op.free()


def _free_bytes():
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_workspace_goes_with_the_other_cg_workspaces(B):
    """600^2 rows (vectors of 2.9 MB: large enough to show in the device's free bytes), kind "none": seven vectors. They are released
    by spmv_amd_pcg_release_workspace() while the operator lives, re-made by the next solve (the same bits), and gone after the
    operator's free(): a release behind it finds nothing to give back."""
    n = 600
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    pc = B.Precond(op, "none")
    b = np.random.default_rng(n).standard_normal(rows)
    first = B.bicgstab_solve(op, m, pc, b, np.zeros(rows), max_iters=3)
    held = _free_bytes()
    B._pcg_lib().spmv_amd_pcg_release_workspace()
    assert _free_bytes() - held >= 7 * rows * 8
    again = B.bicgstab_solve(op, m, pc, b, np.zeros(rows), max_iters=3)
    assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and again[2].iterations == 3
    held = _free_bytes()
    pc.destroy()
    op.free()
    after = _free_bytes()
    assert after - held >= 7 * rows * 8
    B._pcg_lib().spmv_amd_pcg_release_workspace()
    assert _free_bytes() - after < rows * 8


def test_chebyshev_and_multigrid_are_refused(B, capfd):
    n = 33
    A, b, x0 = table_system("grid33")
    m = B.HostMatrix(_csr("grid33")[0], n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    for pc, word in ((B.Precond.chebyshev(op, 2), "chebyshev"), (B.Precond.multigrid(op), "multigrid")):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            B.bicgstab_solve(op, m, pc, b, x0)
        err = capfd.readouterr().err
        assert "[BICGSTAB]" in err and word in err and "symmetric definite" in err
        pc.destroy()
    op.free()


def test_application_solver_flag(B, tmp_path):
    """cg_solver --solver=bicgstab --precond=jacobi on a written .mtx of the 33 grid (b = 1, x0 = 0 are the application's) prints
    the count the restatement takes on that system in both roundings (bicgstab_restatement.APP_CASE); the other kinds and --host
    are refused with a usage sentence; the default print-out on the shipped 81 x 81 file is what --solver=cg prints and what the
    harness test records of that file."""
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    n, iterations = APP_CASE
    A = sp.coo_matrix(convdiff5(n))
    path = tmp_path / "convdiff33.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{A.shape[0]} {A.shape[1]} {A.nnz}\n")
        for r, c, v in zip(A.row, A.col, A.data):
            f.write(f"{r + 1} {c + 1} {float(v)!r}\n")
    js = tmp_path / "out.json"
    for precond, tag in (("jacobi", "cusparse-csr+jacobi+bicgstab"), ("none", "cusparse-csr+bicgstab")):
        out = subprocess.run([exe, str(path), "--mode=cusparse-csr", "--solver=bicgstab", "--precond=" + precond, f"--json={js}"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert f"--- Results for {tag} ---\nConverged: YES in {iterations} iterations" in out.stdout, out.stdout
        assert tag in open(tmp_path / f"out_{tag}.json").read()  # one file per mode string
    for bad in (["--precond=chebyshev"], ["--precond=multigrid:2"], ["--host"], ["--precond=ilu"]):
        out = subprocess.run([exe, str(path), "--solver=bicgstab"] + bad, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--solver=bicgstab" in out.stderr, (bad, out.stderr)
    out = subprocess.run([exe, str(path), "--solver=gmres"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "unknown solver" in out.stderr
    shipped = os.path.join(GOLDEN, "example81x81.mtx")

    def stable(text):  # everything but the timings, and the count of runs the timing statistics kept ("Completed: 9 valid runs, 1 outliers removed")
        return [line for line in text.splitlines() if " ms" not in line and " outliers removed" not in line]

    plain = subprocess.run([exe, shipped], capture_output=True, text=True, timeout=120)
    named = subprocess.run([exe, shipped, "--solver=cg"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and named.returncode == 0 and stable(plain.stdout) == stable(named.stdout)
    # what tests/test_harness.py records of this file: 40 iterations, Sum(x) = -826.08388842537738
    assert "--- Results for stencil5-csr ---\nConverged: YES in 40 iterations" in plain.stdout
    assert abs(float(re.search(r"Sum\(x\):\s+(\S+)", plain.stdout).group(1)) - (-8.2608388842537738e+02)) < 1e-8
    assert "bicgstab" not in plain.stdout.lower() and "Preconditioner" not in plain.stdout
