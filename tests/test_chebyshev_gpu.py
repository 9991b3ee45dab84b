"""The Chebyshev polynomial preconditioner (csrc/precond.hip, its loop in csrc/pcg.hip) on the GPU: the coefficients and the automatic interval
the library reports, the application z = M^-1 r bit for bit against tests/chebyshev_restatement.py on the fused row-lds step and on
the unfused step of every operator, the verdict flag that keeps the converging iteration from streaming, whole solves against the
restatement run with the library's reported interval, and refusals, lifetime and the application's --precond=chebyshev."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import chebyshev_restatement as R
import matrices as M
import pcg_restatement as P
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-10
OPERATORS = ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack")
GUARD = 16
SENTINEL = -6.02214076e23
SUM_TOL = 1e-13  # a re-ordered fp64 sum against math.fsum, of sum|terms| (tests/test_blas1_gpu.py, test_pcg_stages_gpu.py)


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_reset_host_matrices()


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


class Guarded:
    """`values` on the device between GUARD sentinel doubles (the payload stays 16-byte aligned)."""

    def __init__(self, B, values):
        self.n = len(values)
        host = np.full(self.n + 2 * GUARD, SENTINEL)
        host[GUARD:GUARD + self.n] = values
        self.dev = B.DeviceVector.from_host(host)
        self.ptr = self.dev.ptr + 8 * GUARD

    def read(self):
        host = self.dev.to_host()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + self.n:] == SENTINEL), "written outside the array"
        return host[GUARD:GUARD + self.n].copy()

    def free(self):
        self.dev.free()


def stencil_random_values(n, seed=3):
    """matrices.stencil_random_values(n, seed) without its per-entry Python loop (a million rows take it half a minute): the same
    entries in the same order from the same stream of draws -- uniform(a, b) is a + (b - a) * the next double of the generator --,
    checked entry for entry against the original in test_the_matrix_is_the_fixture's."""
    i, j = np.divmod(np.arange(n * n), n)
    present = np.stack([np.ones(n * n, bool), j > 0, j < n - 1, i > 0, i < n - 1], axis=1)  # the writer's order: C, W, E, N, S
    col = np.stack([i * n + j, i * n + j - 1, i * n + j + 1, i * n + j - n, i * n + j + n], axis=1)
    row = np.repeat((i * n + j)[:, None], 5, axis=1)
    u = np.random.default_rng(seed).random(int(present.sum()))
    centre = np.broadcast_to(np.array([True, False, False, False, False]), present.shape)[present]
    e = np.zeros(len(u), dtype=M.ENTRY_DTYPE)
    e["row"], e["col"] = row[present], col[present]
    e["value"] = np.where(centre, 1.0 + (9.0 - 1.0) * u, -2.0 + (2.0 - -2.0) * u)
    return e


def test_the_matrix_is_the_fixtures():
    for n in (3, 40):
        want, rows, cols = M.stencil_random_values(n)
        got = stencil_random_values(n)
        assert rows == cols == n * n and len(got) == len(want)
        for field in ("row", "col", "value"):
            assert np.array_equal(got[field], want[field]), (n, field)


def product_of(O, mode, e, n):
    """The operator's own product order on the CPU."""
    rows = n * n
    rp, ci, va = O.build_csr(e, rows)
    if mode in ("stencil5-csr", "stencil5-ellpack"):
        return lambda v: O.spmv_stencil5(rp, ci, va, v, n)
    if mode == "cusparse-csr":
        return lambda v: O.spmv_csr(rp, ci, va, v)
    w, idx, val = O.build_ell(rp, ci, va)
    return lambda v: O.spmv_ell(rows, w, idx, val, v)


def diagonal_of(e, rows):
    d = np.zeros(rows)
    on = e["row"] == e["col"]
    d[e["row"][on]] = e["value"][on]
    return d


# ---------------------------------------------------------------- info
def test_reported_coefficients_and_interval(B):
    """The coefficients equal the Python recurrence to 4 ulp at degrees 0, 1, 4 and 32 with automatic and explicit bounds; the
    automatic lambda_max equals the restatement's symmetric Gershgorin bound to 4 ulp from all four operators, and is the same bits
    from each; lambda_min = lambda_max / 30."""
    A, _, _ = R.table_system("scaled127")
    n, rows = 127, 127 * 127
    dinv = 1.0 / P.diagonal(A)
    want_hi = R.gershgorin(A, dinv)
    m = B.HostMatrix(P.entries_of(A), rows, rows, n)
    seen = []
    for mode in OPERATORS:
        B.lib().spmv_amd_reset_host_matrices()
        op = B.Operator(mode)
        assert op.init(m) == 0, mode
        for degree in (0, 1, 4, 32):
            for lo, hi in ((0.0, 0.0), (0.05, 2.5), (0.0, 1.9), (0.3, 0.0)):
                pc = B.Precond.chebyshev(op, degree, lo, hi)
                assert pc.kind == "chebyshev"
                got_degree, got_lo, got_hi, coef = pc.chebyshev_info()
                assert got_degree == degree and len(coef) == 1 + 2 * degree
                if hi > 0.0:
                    assert got_hi == hi
                else:
                    assert ulps(got_hi, want_hi) <= 4, (mode, got_hi, want_hi)
                    seen.append(got_hi)
                assert got_lo == (lo if lo > 0.0 else got_hi / 30.0)
                want = R.coefficients(degree, got_lo, got_hi)
                assert max(ulps(g, w) for g, w in zip(coef, want)) <= 4, (mode, degree, lo, hi)
                assert np.array_equal(pc.inverse_diagonal().view(np.uint64), dinv.view(np.uint64)), mode
                few = np.full(3, -1.0)  # a short buffer gets the first `cap` values and the full count
                assert B._pcg_lib().spmv_amd_precond_chebyshev_info(pc.handle, None, None, None, few.ctypes.data, 2) == 1 + 2 * degree
                assert few[2] == -1.0 and few[0] == coef[0] and (degree == 0 or few[1] == coef[1])
                pc.destroy()
        jac = B.Precond(op, "jacobi")
        assert jac.chebyshev_info() is None
        jac.destroy()
        op.free()
    assert len(set(seen)) == 1, set(seen)  # bit-identical among the operators
    assert ulps(seen[0], 1.8) <= 4


# ---------------------------------------------------------------- application, bit for bit
DEGREES = (0, 1, 2, 5)  # both z vectors of the fused step end an application
BOUNDS = (0.1, 3.0)


def check_application(B, O, op, mode, e, n, r, dinv, label):
    rows = n * n
    matvec = product_of(O, mode, e, n)
    out = {}
    dr = Guarded(B, r)
    for degree in DEGREES:
        pc = B.Precond.chebyshev(op, degree, *BOUNDS)
        _, lo, hi, coef = pc.chebyshev_info()
        assert (lo, hi) == BOUNDS
        assert np.array_equal(pc.inverse_diagonal().view(np.uint64), dinv.view(np.uint64)), label
        want = R.make_apply(matvec, dinv, list(coef), fma=O.axpy)(r)  # the library's reported coefficients
        dz = Guarded(B, np.full(rows, np.nan))
        rz = pc.apply_device(op, dr.ptr, dz.ptr)
        z = dz.read()
        assert np.array_equal(z.view(np.uint64), want.view(np.uint64)), (label, degree, int(np.sum(z != want)))
        assert np.array_equal(dr.read(), r), (label, degree)  # the input is only read
        terms = r * want
        err = abs(rz - math.fsum(terms)) / float(np.sum(np.abs(terms)))
        print(f"{label} degree {degree}: r.z err {err:.2e} of sum|terms|")
        assert err <= SUM_TOL, (label, degree, err)
        again = pc.apply_device(op, dr.ptr, dz.ptr)
        assert again == rz and np.array_equal(dz.read().view(np.uint64), z.view(np.uint64)), (label, degree)
        out[degree] = (z, rz)
        dz.free()
        pc.destroy()
    dr.free()
    return out


@pytest.mark.parametrize("n", [3, 65, 127, 512, 513, 640, 1000])
def test_application_on_the_stencil_operator(B, O, n):
    """512: whole tiles, the last ending at column n-1; 513: a fifth tile of one column; 640: whole tiles; 1000: a ragged last tile
    with a partly empty second half; 3, 65, 127: below the row-lds threshold (row-direct, the unfused step). On the row-lds grids
    the fused step and the forced row-direct (unfused) one give the same bits."""
    e = stencil_random_values(n)
    rows = n * n
    dinv = 1.0 / diagonal_of(e, rows)
    r = np.random.default_rng(n).standard_normal(rows)
    m = B.HostMatrix(e, rows, rows, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    try:
        if n >= 512:
            assert op.variant() == "stencil5/row-lds"
            fused = check_application(B, O, op, "stencil5-csr", e, n, r, dinv, f"{n} row-lds")
            assert op.select_variant("row-direct") == 0 and op.variant() == "stencil5/row-direct"
            unfused = check_application(B, O, op, "stencil5-csr", e, n, r, dinv, f"{n} row-direct")
            for degree in DEGREES:
                assert np.array_equal(fused[degree][0].view(np.uint64), unfused[degree][0].view(np.uint64)), degree
        else:
            assert op.variant() == "stencil5/row-direct"
            check_application(B, O, op, "stencil5-csr", e, n, r, dinv, f"{n} row-direct")
    finally:
        op.select_variant(None)
        op.free()


@pytest.mark.parametrize("mode", ["cusparse-csr", "ellpack", "stencil5-ellpack"])
def test_application_on_the_other_operators(B, O, mode):
    """run_device followed by the streaming step, against each operator's own product order; an odd and an even row count."""
    for n in (65, 256):
        B.lib().spmv_amd_reset_host_matrices()
        e = stencil_random_values(n)
        rows = n * n
        dinv = 1.0 / diagonal_of(e, rows)
        r = np.random.default_rng(n).standard_normal(rows)
        op = B.Operator(mode)
        assert op.init(B.HostMatrix(e, rows, rows, n)) == 0
        check_application(B, O, op, mode, e, n, r, dinv, f"{mode} {n}")
        op.free()


def test_kinds_none_and_jacobi_through_the_same_entry_point(B, O):
    for n in (1, 2, 129, 4097):
        rng = np.random.default_rng(n)
        d = rng.uniform(0.5, 4.0, n)
        r = rng.standard_normal(n)
        jac = B.Precond.from_diagonal(d)
        op = B.Operator("cusparse-csr")  # kinds that need no operator: any table of this library passes, initialised or not
        dr, dz = Guarded(B, r), Guarded(B, np.full(n, np.nan))
        rz = jac.apply_device(op, dr.ptr, dz.ptr)
        want = (1.0 / d) * r
        assert np.array_equal(dz.read(), want) and np.array_equal(dr.read(), r)
        assert abs(rz - math.fsum(r * want)) <= SUM_TOL * float(np.sum(np.abs(r * want)))
        assert jac.apply_device(op, dr.ptr, dz.ptr) == rz
        jac.destroy()
        dr.free(), dz.free()
    n = 40
    A = P.stencil5(n)
    op = B.Operator("stencil5-csr")
    assert op.init(B.HostMatrix(P.entries_of(A), n * n, n * n, n)) == 0
    none = B.Precond(op, "none")
    r = np.random.default_rng(4).standard_normal(n * n)
    dr, dz = Guarded(B, r), Guarded(B, np.full(n * n, np.nan))
    rz = none.apply_device(op, dr.ptr, dz.ptr)
    assert np.array_equal(dz.read(), r) and abs(rz - math.fsum(r * r)) <= SUM_TOL * math.fsum(r * r)
    none.destroy()
    dr.free(), dz.free()
    op.free()


# ---------------------------------------------------------------- the verdict flag
def test_the_converging_iteration_runs_no_step(Blab):
    """The steps read the iteration's verdict on the device: the LAB build counts the step launches of the loop that did work, and a
    converged solve has degree * (iterations - 1) of them -- none at all when the first iteration converges. Fused (row-lds) and
    unfused (row-direct) steps."""
    Blab.lib().spmv_amd_reset_host_matrices()
    L = Blab.lib()
    for n, degree in ((127, 4), (512, 3)):
        A, b, x0 = R.table_system(f"poisson{n}")
        op = Blab.Operator("stencil5-csr")
        assert op.init(Blab.HostMatrix(P.entries_of(A), n * n, n * n, n)) == 0
        assert op.variant() == ("stencil5/row-lds" if n >= 512 else "stencil5/row-direct")
        pc = Blab.Precond.chebyshev(op, degree)
        _, _, st = Blab.pcg_solve_device(op, Blab.HostMatrix(P.entries_of(A), n * n, n * n, n), pc, b, x0, tol=1e-2)
        assert st.converged == 1 and st.iterations >= 1
        first = st.iterations
        assert L.spmv_amd_pcg_last_step_launches() == degree * (first - 1)
        _, _, st = Blab.pcg_solve_device(op, Blab.HostMatrix(P.entries_of(A), n * n, n * n, n), pc, b, x0, tol=1e30)
        assert st.converged == 1 and st.iterations == 1 and L.spmv_amd_pcg_last_step_launches() == 0
        _, _, st = Blab.pcg_solve_device(op, Blab.HostMatrix(P.entries_of(A), n * n, n * n, n), pc, b, x0, max_iters=7, tol=1e-12)
        assert st.converged == 0 and st.iterations == 7 and L.spmv_amd_pcg_last_step_launches() == degree * 7
        jac = Blab.Precond(op, "jacobi")
        Blab.pcg_solve_device(op, Blab.HostMatrix(P.entries_of(A), n * n, n * n, n), jac, b, x0, max_iters=3)
        assert L.spmv_amd_pcg_last_step_launches() == 0
        jac.destroy()
        pc.destroy()
        op.free()
        Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- whole solves
SOLVES = [("poisson127", 2, 1e-6, 107), ("poisson127", 4, 1e-6, 69), ("poisson127", 8, 1e-6, 45), ("poisson255", 4, 1e-6, 136),
          ("poisson513", 4, 1e-6, 261), ("scaled127", 4, 1e-6, 8), ("negated65", 4, 1e-6, 8), ("scaled601", 4, 1e-6, 8),
          ("plain601", 2, 1e-6, 13), ("poisson127", 4, 1e-10, 95)]


def solve_and_compare(B, op, m, A, b, x0, degree, tol, iterations, label):
    pc = B.Precond.chebyshev(op, degree)
    _, lo, hi, _ = pc.chebyshev_info()
    xo, ho, ito, conv = R.pcg(A, b, x0, degree, lo, hi, tol, 1000)  # the restatement with the library's reported interval
    assert conv and ito == iterations, (label, ito)
    x, h, st = B.pcg_solve_device(op, m, pc, b, x0, tol=tol)
    err = P.hist_err(h, ho)
    print(f"{label}: {st.iterations} iterations, history {err:.2e}, x {np.max(np.abs(x - xo)) / np.max(np.abs(xo)):.2e}")
    assert st.converged == 1 and st.iterations == iterations, (label, st.iterations)
    assert len(h) == iterations + 1 and err < TOL, (label, err)
    assert np.max(np.abs(x - xo)) <= 1e-8 * np.max(np.abs(xo)), label
    assert P.true_residual_norm(P.entries_of(A), b, x) < tol * h[0] * (1.0 + 1e-6), label
    x2, h2, _ = B.pcg_solve_device(op, m, pc, b, x0, tol=tol)
    assert np.array_equal(x2, x) and np.array_equal(h2, h), label  # fixed-shape sums: the same bits
    pc.destroy()


@pytest.mark.parametrize("name,degree,tol,iterations", SOLVES)
def test_whole_solves_against_the_restatement(B, name, degree, tol, iterations):
    A, b, x0 = R.table_system(name)
    n = int(round(math.sqrt(A.shape[0])))
    m = B.HostMatrix(P.entries_of(A), n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    assert op.variant() == ("stencil5/row-lds" if n >= 512 else "stencil5/row-direct")  # poisson513, the 601s: the fused step
    solve_and_compare(B, op, m, A, b, x0, degree, tol, iterations, f"{name} degree {degree} tol {tol}")
    op.free()


@pytest.mark.parametrize("mode", ["cusparse-csr", "ellpack", "stencil5-ellpack"])
def test_whole_solves_on_the_other_operators(B, mode):
    for name, degree, tol, iterations in (("scaled127", 4, 1e-6, 8), ("poisson127", 8, 1e-6, 45)):
        B.lib().spmv_amd_reset_host_matrices()
        A, b, x0 = R.table_system(name)
        m = B.HostMatrix(P.entries_of(A), 127 * 127, 127 * 127, 127)
        op = B.Operator(mode)
        assert op.init(m) == 0
        solve_and_compare(B, op, m, A, b, x0, degree, tol, iterations, f"{mode} {name} degree {degree}")
        op.free()


def test_degree_zero_is_jacobi_and_degree_four_cuts_iterations_threefold(B):
    """Degree 0 reproduces the Jacobi history of the same system to 1e-10; poisson127 at degree 4 needs fewer than a third of
    Jacobi's iterations, both run on the GPU."""
    for name in ("scaled127", "poisson127"):
        B.lib().spmv_amd_reset_host_matrices()
        A, b, x0 = R.table_system(name)
        m = B.HostMatrix(P.entries_of(A), 127 * 127, 127 * 127, 127)
        op = B.Operator("stencil5-csr")
        assert op.init(m) == 0
        jac, zero, four = B.Precond(op, "jacobi"), B.Precond.chebyshev(op, 0), B.Precond.chebyshev(op, 4)
        xj, hj, sj = B.pcg_solve_device(op, m, jac, b, x0)
        x0_, h0, s0 = B.pcg_solve_device(op, m, zero, b, x0)
        assert sj.converged == 1 and s0.converged == 1 and s0.iterations == sj.iterations and P.hist_err(h0, hj) < TOL, name
        assert np.max(np.abs(x0_ - xj)) <= 1e-8 * np.max(np.abs(xj))
        if name == "poisson127":
            _, _, s4 = B.pcg_solve_device(op, m, four, b, x0)
            assert s4.converged == 1 and 3 * s4.iterations < sj.iterations, (s4.iterations, sj.iterations)
        for pc in (jac, zero, four):
            pc.destroy()
        op.free()


def timers_change_no_bit(B, op, m, pc, b, x0, label):
    """enable_detailed_timers = 1 (events between the launches) against the plain solve: x and the history bit for bit and the same
    iteration count; the timed solve reports each of the three stage times > 0 and their sum <= the total, the plain one reports the
    three as 0 (tests/test_pcg_gpu.py asserts the same of the Jacobi loop)."""
    x, h, st = B.pcg_solve_device(op, m, pc, b, x0)
    xt, ht, stt = B.pcg_solve_device(op, m, pc, b, x0, timers=1)
    print(f"{label}: {st.iterations} iterations; timed: spmv {stt.time_spmv_ms:.3f} blas1 {stt.time_blas1_ms:.3f} "
          f"reductions {stt.time_reductions_ms:.3f} of {stt.time_total_ms:.3f} ms")
    assert np.array_equal(xt, x) and np.array_equal(ht, h) and stt.iterations == st.iterations and stt.converged == 1, label
    assert st.time_spmv_ms == 0.0 and st.time_blas1_ms == 0.0 and st.time_reductions_ms == 0.0 and st.time_total_ms > 0.0, label
    assert stt.time_spmv_ms > 0.0 and stt.time_blas1_ms > 0.0 and stt.time_reductions_ms > 0.0, label
    assert stt.time_spmv_ms + stt.time_blas1_ms + stt.time_reductions_ms <= stt.time_total_ms, label


@pytest.mark.parametrize("mode,n,rowlds_from", [("stencil5-csr", 130, 64), ("stencil5-csr", 130, None), ("ellpack", 65, None)])
def test_detailed_timers_change_no_bit(B, monkeypatch, mode, n, rowlds_from):
    """Degree 2 on the three forms of a step: the fused row-lds launch (the row-lds threshold lowered to 64), the stencil operator's
    SpMV behind the device flag + the streaming step (the default threshold: row-direct), and run_device + the streaming step."""
    if rowlds_from is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", str(rowlds_from))
    rows = n * n
    A = P.stencil5(n, center=4.0)
    m = B.HostMatrix(P.entries_of(A), rows, rows, n)
    op = B.Operator(mode)
    assert op.init(m) == 0
    if mode == "stencil5-csr":
        assert op.variant() == ("stencil5/row-lds" if rowlds_from is not None else "stencil5/row-direct")
    pc = B.Precond.chebyshev(op, 2)
    b = np.random.default_rng(n).standard_normal(rows)
    timers_change_no_bit(B, op, m, pc, b, np.zeros(rows), f"{mode} {n} row-lds from {rowlds_from}")
    pc.destroy()
    op.free()


@pytest.mark.parametrize("case", ["81:5.0", "81:-4.0", "512:5.0"])
def test_golden_anchors_at_degree_zero(B, O, case):
    gold = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["cases"][case]["cg"]
    n, center = int(case.split(":")[0]), float(case.split(":")[1])
    op = B.Operator("stencil5-csr")
    if n >= 512:
        assert op.init_synthetic(n) == 0
        m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n * n, n * n, n)
    else:
        m = B.HostMatrix(O.stencil5_coo(n, center, -1.0), n * n, n * n, n)
        assert op.init(m) == 0
    pc = B.Precond.chebyshev(op, 0)
    _, h, st = B.pcg_solve_device(op, m, pc, np.ones(n * n), np.zeros(n * n))
    assert st.converged == 1 and st.iterations == gold["iterations"], (case, st.iterations)
    assert P.hist_err(h, np.array(gold["history"])) < TOL, case
    assert abs(st.solution_sum - gold["solution_sum"]) <= 1e-9 * abs(gold["solution_sum"])
    pc.destroy()
    op.free()


# ---------------------------------------------------------------- refusals and lifetime
def test_refusals_on_the_device(B):
    n = 40
    rows = n * n
    A = P.stencil5(n)
    e = P.entries_of(A)
    m = B.HostMatrix(e, rows, rows, n)
    b = np.ones(rows)
    op, other = B.Operator("stencil5-csr"), B.Operator("cusparse-csr")
    assert op.init(m) == 0 and other.init(m) == 0
    pc = B.Precond.chebyshev(op, 3)
    dr, dz = B.DeviceVector.from_host(b), B.DeviceVector(rows, fill=0.0)
    assert pc.apply_device(op, dr.ptr, dz.ptr) != 0.0
    for r_ptr, z_ptr in ((dr.ptr, dr.ptr), (dr.ptr, dr.ptr + 16), (dr.ptr + 16 * 10, dr.ptr)):  # d_z == d_r, and overlaps
        with pytest.raises(RuntimeError):
            pc.apply_device(op, r_ptr, z_ptr)
    with pytest.raises(RuntimeError):  # a foreign preconditioner
        pc.apply_device(other, dr.ptr, dz.ptr)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(other, m, pc, b, np.zeros(rows))
    for lo, hi in ((1.9, 0.0), (5.0, 0.0)):  # an explicit lambda_min at or above the automatic lambda_max (1.8)
        with pytest.raises(ValueError) as info:
            B.Precond.chebyshev(op, 3, lo, hi)
        assert info.value.bad_row == -1
    assert op.init(m) == 0  # a stale one: made before the operator was last initialised
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
    with pytest.raises(RuntimeError):
        pc.apply_device(op, dr.ptr, dz.ptr)
    pc.destroy()
    fresh = B.Precond.chebyshev(op, 3)
    _, _, st = B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
    assert st.converged == 1
    op.free()
    with pytest.raises(RuntimeError):  # after free()
        B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
    fresh.destroy()
    other.free()
    dr.free(), dz.free()
    # a bad diagonal row: bad_row as for Jacobi (zero, of the other sign, not finite)
    for value in (0.0, -5.0, float("inf")):
        B.lib().spmv_amd_reset_host_matrices()
        bad = e.copy()
        at = np.nonzero((bad["row"] == 777) & (bad["col"] == 777))[0][0]
        bad["value"][at] = value
        for mode in ("stencil5-csr", "ellpack"):
            B.lib().spmv_amd_reset_host_matrices()
            o = B.Operator(mode)
            assert o.init(B.HostMatrix(bad, rows, rows, n)) == 0
            with pytest.raises(ValueError) as info:
                B.Precond.chebyshev(o, 2)
            assert info.value.bad_row == 777, (mode, value)
            o.free()


def _free_bytes():
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_coexistence_and_workspace_release(B):
    """cg_solve_device, a Jacobi solve and a Chebyshev solve in one process leave each other's results alone, and the Chebyshev
    vectors (d, z, z' on top of the five every kind keeps) go back to the device with every release entry point."""
    n = 1000
    rows = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, n)
    b = np.random.default_rng(8).standard_normal(rows)
    zero = np.zeros(rows)
    jac, cheb = B.Precond(op, "jacobi"), B.Precond.chebyshev(op, 2)
    runs = {}
    for round_ in range(2):
        for name, solve in (("cg", lambda: B.cg_solve(op, m, b, zero)), ("jacobi", lambda: B.pcg_solve_device(op, m, jac, b, zero)),
                            ("chebyshev", lambda: B.pcg_solve_device(op, m, cheb, b, zero))):
            x, h, st = solve()
            assert st.converged == 1, name
            if round_ == 0:
                runs[name] = (x, h)
            else:
                assert np.array_equal(runs[name][0], x) and np.array_equal(runs[name][1], h), name
    assert P.hist_err(runs["jacobi"][1], runs["cg"][1]) < TOL  # a constant diagonal: Jacobi is plain CG
    assert len(runs["chebyshev"][1]) < len(runs["jacobi"][1])
    vectors = 8 * rows * 8  # x, b, r, p, Ap and d, z, z'
    releases = (B.lib().spmv_amd_cg_release_workspace, B._pcg_lib().spmv_amd_pcg_release_workspace, None)
    for release in releases:
        B.pcg_solve_device(op, m, cheb, b, zero)
        held = _free_bytes()
        if release is None:
            jac.destroy(), cheb.destroy()
            after_destroy = _free_bytes()
            op.free()
            assert _free_bytes() - after_destroy >= vectors
        else:
            release()
            assert _free_bytes() - held >= vectors, release
            release()  # nothing held: a no-op
    B.lib().spmv_amd_reset_host_matrices()


def test_application_chebyshev_flag(B):
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    out = subprocess.run([exe, "--stencil=512", "--precond=chebyshev:3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--- Results for stencil5-csr+chebyshev3 ---\nConverged: YES in " in out.stdout, out.stdout
    out = subprocess.run([exe, "--stencil=512", "--precond=chebyshev:99"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "chebyshev" in out.stderr
