"""GCR(m) (spmv_amd_gcr_solve_device, csrc/gcr.hip) on the GPU: whole solves of the nonsymmetric table systems under every kind of
preconditioner, BIT for bit against gcr_restatement.gcr_exact -- the operator's own product, the dots as the kernels sum them, every
update an fma, the application of kinds "chebyshev" and "multigrid" the library's own spmv_amd_precond_apply_device (held bit for bit
to the restatement's oracle form here as well, on these nonsymmetric matrices) -- and within the row's third-rounding bound of plain
numpy; the 3-D twin with its own hierarchy; every other operator on ITS product; the breakdowns; determinism; the workspace's life;
the refusals the other solvers keep; and the application's --solver=gcr[:m] (tests/test_gcr_stages_gpu.py has the kernels one by one,
tests/test_gcr_host.py the soundness of the inputs)."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gcr_restatement as G
from conftest import ROOT
from gcr_restatement import APP_CASE, TABLE, convdiff5, entries_of, hist_err, table_system, third_rounding_bound

pytestmark = pytest.mark.gpu
ROWLDS_KNOB = "SPMV_AMD_ROWLDS_MIN_GRID"
FLAT = [i for i, r in enumerate(TABLE) if G.dimension_of(r[0]) == 2]
CUBE = [i for i, r in enumerate(TABLE) if G.dimension_of(r[0]) == 3]
# kinds the table does not carry on the 2-D systems: held to the exact form alone, over a fixed number of iterations
EXTRA = [("grid33", "jacobi", 4), ("grid33", "chebyshev2", 4), ("grid65", "chebyshev4", 16), ("rows127", "chebyshev3", 16), ("grid65", "multigrid2", 1),
         ("grid33", "multigrid0", 32), ("grid127", "jacobi", 0)]


def row_id(i):
    return f"{TABLE[i][0]}-{TABLE[i][1]}-m{TABLE[i][2]}-{TABLE[i][3]:g}"


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


def product_of(name, family):
    """The product of one operator family on a table system: "stencil5" (oracle.spmv_stencil5: stencil5-csr in all its variants,
    stencil5-ellpack) or "csr" (oracle.spmv_csr: the sequential CSR kernels, ellpack, stencil7-csr)."""
    from oracle import oracle as O

    A, _, _ = table_system(name)
    _, rp, ci, va = _csr(name)
    grid = int(round(np.sqrt(A.shape[0])))
    return (lambda u: O.spmv_stencil5(rp, ci, va, u, grid)) if family == "stencil5" else (lambda u: O.spmv_csr(rp, ci, va, u))


def make_precond(B, op, kind, dim):
    name, k = G.parse_kind(kind)
    if name == "chebyshev":
        return B.Precond.chebyshev(op, k)
    if name == "multigrid":
        return B.Precond.multigrid(op, k) if dim == 2 else B.Precond.multigrid3d(op, k)
    return B.Precond(op, name)


class DeviceApply:
    """r -> z = M^-1 r through spmv_amd_precond_apply_device on two device vectors of its own."""

    def __init__(self, B, op, pc, n):
        self.B, self.op, self.pc = B, op, pc
        self.r, self.z = B.DeviceVector(n, 0.0), B.DeviceVector(n, 0.0)

    def __call__(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        self.B.lib().spmv_amd_copy_to_device(self.r.ptr, r.ctypes.data, r.nbytes)
        self.pc.apply_device(self.op, self.r.ptr, self.z.ptr)
        return self.z.to_host()

    def free(self):
        self.r.free(), self.z.free()


def exact_application(B, op, pc, kind, A):
    """The application gcr_exact is given: for "none" and "jacobi" the statement itself, else the library's own."""
    name, _ = G.parse_kind(kind)
    if name == "none":
        return (lambda r: r), None
    if name == "jacobi":
        dinv = 1.0 / G.diagonal(A)
        return (lambda r: dinv * r), None
    a = DeviceApply(B, op, pc, A.shape[0])
    return a, a


def check_exact(got, want, what):
    """(x, history, stats) of the device against (x, history, iterations, converged, end) of the exact form, bit for bit"""
    x, h, st = got
    wx, wh, wit, wconv, _ = want
    assert (st.iterations, st.converged) == (wit, int(wconv)) and len(h) == len(wh), (what, st.iterations, st.converged, wit, wconv)
    diff = np.flatnonzero(np.ascontiguousarray(h).view(np.uint64) != np.ascontiguousarray(wh).view(np.uint64))
    assert len(diff) == 0, (what, "history differs first at", int(diff[0]), float(h[diff[0]]), float(wh[diff[0]]))
    assert same_bits(x, wx), (what, float(np.max(np.abs(x - wx))))


def solve_and_exact(B, name, kind, restart, tol, mode, family, max_iters=1000, variant=None, expect_variant=None):
    """One solve on the device and the exact form of the same solve; returns (got, want)."""
    A, b, x0 = table_system(name)
    dim = G.dimension_of(name)
    m = B.HostMatrix(_csr(name)[0], A.shape[0], A.shape[0], G.grid_of(A, dim))
    op = B.Operator(mode)
    if variant is not None and mode != "stencil5-csr":  # the CSR operator's variant is chosen at init, the stencil operator's after it
        assert op.select_variant(variant) == 0
    try:
        assert op.init(m) == 0, mode
        if variant is not None and mode == "stencil5-csr":
            assert op.select_variant(variant) == 0
        if expect_variant is not None:
            assert op.variant() == expect_variant, op.variant()
        pc = make_precond(B, op, kind, dim)
        try:
            got = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol, max_iters=max_iters)
            apply, owned = exact_application(B, op, pc, kind, A)
            try:
                want = G.gcr_exact(product_of(name, family), b, x0, apply, restart, tol, max_iters)
            finally:
                if owned is not None:
                    owned.free()
            return got, want
        finally:
            pc.destroy()
    finally:
        op.free()
        if variant is not None:
            op.select_variant(None)


def check_row(B, row, mode, family, what, **kw):
    name, kind, restart, tol, iterations, stored = TABLE[row]
    got, want = solve_and_exact(B, name, kind, restart, tol, mode, family, **kw)
    assert want[2] == iterations and want[3], (what, want[2:])
    check_exact(got, want, what)
    x, h, st = got
    xp, hp, _, _, _ = G.two_roundings(name, kind, restart, tol)[0]
    bound = third_rounding_bound(stored)
    err = hist_err(h, hp)
    print(f"{what}: {st.iterations} iterations, device against plain numpy {err:.2e} (bound {bound:.0e})")
    assert err <= bound and np.max(np.abs(x - xp)) <= bound * np.max(np.abs(xp)), (what, err)
    assert st.residual_norm == h[-1] and h[-1] / h[0] < tol <= h[-2] / h[0]
    assert np.max(np.diff(h)) <= 1e-12 * h[0]
    return got


@pytest.mark.parametrize("row", FLAT, ids=row_id)
def test_table_rows_on_stencil5_csr_row_direct_bit_for_bit(B, row):
    check_row(B, row, "stencil5-csr", "stencil5", row_id(row), expect_variant="stencil5/row-direct")


@pytest.mark.parametrize("name,kind,restart", EXTRA, ids=[f"{e[0]}-{e[1]}-m{e[2]}" for e in EXTRA])
def test_every_kind_on_the_2d_systems_bit_for_bit(B, name, kind, restart):
    """"jacobi" on a constant diagonal, "chebyshev" of three degrees, "multigrid" with nu = 0 and 2, restart 1, 32 and the default:
    14 iterations each under a tolerance that is never met."""
    got, want = solve_and_exact(B, name, kind, restart, 1e-300, "stencil5-csr", "stencil5", max_iters=14, expect_variant="stencil5/row-direct")
    assert want[2] == 14 and not want[3]
    check_exact(got, want, (name, kind, restart))
    assert np.max(np.diff(got[1])) <= 1e-12 * got[1][0]


def test_a_row_lds_solve_bit_for_bit(B):
    """601^2 rows (row-lds by itself; 2822 partials: the two-stage reduction), "jacobi", m = 4, 12 iterations: three restarts."""
    got, want = solve_and_exact(B, "grid601", "jacobi", 4, 1e-300, "stencil5-csr", "stencil5", max_iters=12, expect_variant="stencil5/row-lds")
    assert want[2] == 12 and not want[3] and got[2].residual_norm == got[1][0]  # unconverged without verbose: ||r0|| is reported
    check_exact(got, want, "grid601")


@pytest.mark.parametrize("kind", ["chebyshev2", "multigrid1"])
def test_row_lds_applications_inside_the_loop(B, monkeypatch, kind):
    """The fused Chebyshev step and the row-lds levels of a hierarchy, forced on the 65 grid: 10 iterations bit for bit."""
    monkeypatch.setenv(ROWLDS_KNOB, "8")
    got, want = solve_and_exact(B, "grid65", kind, 4, 1e-300, "stencil5-csr", "stencil5", max_iters=10, expect_variant="stencil5/row-lds")
    check_exact(got, want, kind)


@pytest.mark.parametrize("row", CUBE, ids=row_id)
def test_stencil7_csr_on_the_3d_twin(B, row):
    """cube16 under "none", "chebyshev2" and the 3-D hierarchy (spmv_amd_precond_create_multigrid3d)."""
    check_row(B, row, "stencil7-csr", "csr", row_id(row))


OTHERS = [("stencil5-csr", "row-generic", "stencil5/row-generic", "stencil5"), ("stencil5-ellpack", None, "ell/stencil5-direct", "stencil5"),
          ("cusparse-csr", "stream", "csr/stream", "csr"), ("cusparse-csr", "row-scalar", "csr/row-scalar", "csr"),
          ("ellpack", None, "ell/slot-major", "csr")]


@pytest.mark.parametrize("mode,variant,variant_name,family", OTHERS, ids=[o[2] for o in OTHERS])
def test_every_operator_gives_the_bits_of_its_own_product(B, mode, variant, variant_name, family):
    """Every dot product of the solve is a streaming sum, whatever the operator: the only thing an operator contributes is the bits
    of A z. grid33, "none", m = 4 at tol 1e-6 on each."""
    row = next(i for i in FLAT if TABLE[i][:4] == ("grid33", "none", 4, 1e-6))
    check_row(B, row, mode, family, variant_name, variant=variant, expect_variant=variant_name)


def test_the_applications_are_the_restatements_on_nonsymmetric_matrices(B, O):
    """What exact_application borrows from the library, held to the restatement's oracle form (gcr_restatement.exact_apply on the
    library's reported lambda_max) bit for bit on the upwind matrices: the Chebyshev application and the V-cycle in 2-D and 3-D."""
    for name, mode, kind in (("grid33", "stencil5-csr", "chebyshev2"), ("grid33", "stencil5-csr", "multigrid1"),
                             ("cube16", "stencil7-csr", "multigrid1"), ("cube16", "stencil7-csr", "chebyshev2")):
        A, b, _ = table_system(name)
        dim = G.dimension_of(name)
        m = B.HostMatrix(_csr(name)[0], A.shape[0], A.shape[0], G.grid_of(A, dim))
        op = B.Operator(mode)
        assert op.init(m) == 0
        pc = make_precond(B, op, kind, dim)
        lmax = pc.chebyshev_info()[2] if kind.startswith("chebyshev") else pc.multigrid_info()[2]
        theirs = DeviceApply(B, op, pc, A.shape[0])
        ours = G.exact_apply(O, A, dim, kind, lambda_max=lmax)
        assert same_bits(theirs(b), ours(b)), (name, kind)
        theirs.free()
        pc.destroy()
        op.free()


def _entries(B, triples):
    e = np.zeros(len(triples), dtype=B.ENTRY_DTYPE)
    for k, v in enumerate(triples):
        e[k] = v
    return e


def test_breakdowns_end_with_x_untouched(B, capfd):
    """A = 0 I (stored zeros) under a caller's diagonal (spmv_amd_precond_create_from_diagonal): z = dinv r is an ordinary vector,
    q = A z = 0, gamma = 0 -- iteration 1 is counted, the unchanged residual recorded, x = x0 bit for bit, converged = 0. A quarter
    turn, b = (1, 0): q = (0, -1) is orthogonal to r, rho = 0 with gamma = 1 -- the same ending. Both equal the exact form."""
    from oracle import oracle as O

    cases = ((_entries(B, [(i, i, 0.0) for i in range(5)]), np.array([1.5, -0.75, 2.0, 0.5, -1.0]), np.array([0.25, 0.5, -1.0, 3.0, 0.125]),
              np.full(5, 2.0), "gamma"),
             (_entries(B, [(0, 1, 1.0), (1, 0, -1.0)]), np.array([1.0, 0.0]), np.zeros(2), None, "rho"))
    for e, b, x0, diag, end in cases:
        n = len(b)
        B.lib().spmv_amd_reset_host_matrices()
        m = B.HostMatrix(e, n, n, -1)
        op = B.Operator("cusparse-csr")
        assert op.init(m) == 0
        pc = B.Precond.from_diagonal(diag) if diag is not None else B.Precond(op, "none")
        capfd.readouterr()
        x, h, st = B.gcr_solve(op, m, pc, b, x0, restart=4, verbose=1)
        out = capfd.readouterr().out
        rp, ci, va = O.build_csr(e, n)
        apply = (lambda r: r) if diag is None else (lambda r: (1.0 / diag) * r)
        want = G.gcr_exact(lambda u: O.spmv_csr(rp, ci, va, u), b, x0, apply, 4)
        assert want[4] == end and want[2] == 1
        check_exact((x, h, st), want, end)
        assert same_bits(x, x0) and st.iterations == 1 and st.converged == 0 and len(h) == 2 and same_bits(h[1:], h[:1]) and h[0] > 0.0
        assert f"[GCR-DEVICE] Breakdown in iteration 1 ({end} = " in out and "[GCR-DEVICE] Converged: NO" in out
        pc.destroy()
        op.free()


def test_determinism_timers_statistics_and_the_other_solvers(B, capfd):
    """A solve run twice is bit-identical (with the detailed timers too, and after solves of other kinds and restarts in between);
    max_iters = 0 returns x0; a capped solve's history is the full one's beginning; verbose 2 reports the last residual; PCG's and
    BiCGSTAB's histories are left alone; BiCGSTAB still refuses a multigrid handle, before and after a GCR solve with it."""
    name, kind, restart, tol = "grid65", "multigrid1", 4, 1e-6
    iterations = next(r[4] for r in TABLE if r[:4] == (name, kind, restart, tol))
    A, b, x0 = table_system(name)
    rows = A.shape[0]
    m = B.HostMatrix(_csr(name)[0], rows, rows, 65)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    pc, jac = B.Precond.multigrid(op, 1), B.Precond(op, "jacobi")

    def bicgstab_refuses():
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            B.bicgstab_solve(op, m, pc, b, x0)
        err = capfd.readouterr().err
        assert "[BICGSTAB]" in err and "multigrid" in err and "symmetric definite" in err

    bicgstab_refuses()
    first = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol)
    bicgstab_refuses()
    _, hb, _ = B.bicgstab_solve(op, m, jac, b, x0)
    _, hp, _ = B.pcg_solve_device(op, m, jac, b, x0, max_iters=5)
    B.gcr_solve(op, m, jac, b, x0, restart=16, max_iters=20)
    again = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol)
    timed = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol, timers=1)
    for other in (again, timed):
        assert same_bits(other[0], first[0]) and same_bits(other[1], first[1]) and other[2].iterations == iterations
    st, stt = first[2], timed[2]
    assert st.converged == 1 and st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0
    assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0
    assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms
    assert abs(st.solution_sum - np.sum(first[0])) <= 1e-9 * np.sum(np.abs(first[0]))
    for lib_fn, h in ((B._pcg_lib().spmv_amd_pcg_last_history, hp), (B._pcg_lib().spmv_amd_bicgstab_last_history, hb)):
        lib_fn.argtypes = [C.c_void_p, C.c_int]
        out = np.zeros(len(h) + 1)
        assert lib_fn(out.ctypes.data, len(out)) == len(h) and same_bits(out[:len(h)], h)
    x, h, st0 = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol, max_iters=0)
    assert st0.iterations == 0 and st0.converged == 0 and len(h) == 1 and same_bits(x, x0) and same_bits(h, first[1][:1])
    x5, h5, st5 = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol, max_iters=5)
    assert st5.iterations == 5 and st5.converged == 0 and same_bits(h5, first[1][:6]) and st5.residual_norm == h5[0]
    capfd.readouterr()
    x5v, h5v, st5v = B.gcr_solve(op, m, pc, b, x0, restart=restart, tol=tol, max_iters=5, verbose=2)
    out = capfd.readouterr().out
    assert same_bits(x5v, x5) and same_bits(h5v, h5) and st5v.residual_norm == h5v[5]
    assert len(re.findall(r"\[GCR-DEVICE\] Iter +\d+: residual", out)) == 5 and "[GCR-DEVICE] Initial residual" in out and "[PCG" not in out
    # a caller's own operator table with a caller's diagonal: the bits of the "jacobi" solve
    mine = B.gcr_solve(op, m, jac, b, x0, restart=restart, max_iters=9)
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: op.op.contents.run_device(dx, dy))
    foreign = type("Foreign", (), {"op": C.pointer(own)})()
    pd = B.Precond.from_diagonal(np.asarray(A.diagonal()))
    theirs = B.gcr_solve(foreign, m, pd, b, x0, restart=restart, max_iters=9)
    assert same_bits(theirs[0], mine[0]) and same_bits(theirs[1], mine[1])
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        B.gcr_solve(foreign, m, pc, b, x0)  # pc belongs to `op`
    with pytest.raises(RuntimeError):
        B.gcr_solve(op, m, pc, b, x0, restart=33)
    assert "restart = 33" in capfd.readouterr().err
    for p in (pd, pc, jac):
        p.destroy()
    op.free()


def _free_bytes():
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_workspace_goes_with_the_other_cg_workspaces(B):
    """600^2 rows (vectors of 2.9 MB: large enough to show in the device's free bytes). A release gives back at least what
    spmv_amd_gcr_workspace_bytes promised for the restart and kind of the solve; the next solve makes it again (the same bits); after
    the operator's free() a release finds nothing to give back."""
    n = 600
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    b = np.random.default_rng(n).standard_normal(rows)
    for kind, restart in (("none", 4), ("jacobi", 16), ("chebyshev", 2)):
        pc = B.Precond.chebyshev(op, 2) if kind == "chebyshev" else B.Precond(op, kind)
        promised = B.gcr_workspace_bytes(rows, restart, kind)
        assert promised >= (3 + 2 * restart) * rows * 8
        B._pcg_lib().spmv_amd_pcg_release_workspace()
        first = B.gcr_solve(op, m, pc, b, np.zeros(rows), restart=restart, max_iters=3)
        held = _free_bytes()
        B._pcg_lib().spmv_amd_pcg_release_workspace()
        given = _free_bytes() - held
        # at least what was promised; the allocator's granularity, the history and the reduction scratch come on top
        assert promised <= given < 2 * promised + (64 << 20), (kind, restart, promised, given)
        again = B.gcr_solve(op, m, pc, b, np.zeros(rows), restart=restart, max_iters=3)
        assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and again[2].iterations == 3
        pc.destroy()
    held = _free_bytes()
    op.free()
    after = _free_bytes()
    assert after - held >= B.gcr_workspace_bytes(rows, 2, "chebyshev")
    B._pcg_lib().spmv_amd_pcg_release_workspace()
    assert _free_bytes() - after < rows * 8


def test_application_solver_flag(B, tmp_path):
    """cg_solver --solver=gcr:4 --precond=multigrid on a written .mtx of the 33 grid (b = 1, x0 = 0 are the application's) converges
    in the count the restatement takes on that system in every rounding (gcr_restatement.APP_CASE) and names its mode string in the
    JSON; a malformed restart and --host are refused with a sentence; --solver=gmres is still unknown; --solver=bicgstab still turns
    --precond=multigrid away."""
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    n, restart, kind, iterations = APP_CASE
    A = sp.coo_matrix(convdiff5(n))
    path = tmp_path / "convdiff33.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"% STENCIL_GRID_SIZE {n}\n")  # the comment the operators read: without it the file is a general CSR, no stencil
        f.write(f"{A.shape[0]} {A.shape[1]} {A.nnz}\n")
        for r, c, v in zip(A.row, A.col, A.data):
            f.write(f"{r + 1} {c + 1} {float(v)!r}\n")
    js = tmp_path / "out.json"
    tag = f"stencil5-csr+{kind}+gcr{restart}"
    out = subprocess.run([exe, str(path), f"--solver=gcr:{restart}", "--precond=multigrid", f"--json={js}"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"--- Results for {tag} ---\nConverged: YES in {iterations} iterations" in out.stdout, out.stdout
    text = open(tmp_path / f"out_{tag}.json").read()
    assert tag in text and json.loads(text) is not None
    out = subprocess.run([exe, str(path), "--solver=gcr", "--maxiter=3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--- Results for stencil5-csr+gcr16 ---\nConverged: NO in 3 iterations" in out.stdout, out.stdout + out.stderr
    for bad, word in ((["--solver=gcr:0x"], "--solver=gcr:M"), (["--solver=gcr:33"], "--solver=gcr:M"), (["--solver=gcr:0"], "--solver=gcr:M"),
                      (["--solver=gcr:"], "--solver=gcr:M"), (["--solver=gcr:4", "--host"], "--solver=gcr"),
                      (["--solver=gcr:4", "--precond=ilu"], "unknown preconditioner"), (["--solver=gmres"], "unknown solver"),
                      (["--solver=gcrx"], "unknown solver"), (["--solver=bicgstab", "--precond=multigrid"], "--solver=bicgstab")):
        out = subprocess.run([exe, str(path)] + bad, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and word in out.stderr and out.stderr.count("\n") == 1, (bad, out.stderr)
