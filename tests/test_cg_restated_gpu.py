"""Whole CG solves equal to the numpy restatement of the loop (tests/cg_restatement.py), bit for bit: every entry of the residual
history, the iteration count, the verdict and x. The forms of the library already agree with each other bit for bit (ring 1 / 16,
pipeline / plain, block rows, planes / CSR coefficients, run-ahead); this says what those bits are. The sums come from
tests/reduction_restatement.py, so a partial in the wrong slot, extras in another place of the second stage, or a re-shaped tree
shows here as a history that differs in its last bits -- random coefficients and vectors, so that no two slots hold equal data.
The second half puts the stopping test sqrt(rr_new) / b_norm < tol on its edge: the tolerance equal to a ratio of the solve's own
history goes on, the next double above it stops there."""
import numpy as np
import pytest

import cg_restatement as CG
from bitwise import same_bits
from test_symmetric_coefficients_gpu import symmetric_coo

pytestmark = pytest.mark.gpu

TOL, MAX_ITERS = 1e-8, 300
# n, coefficients, SPMV_AMD_ROWLDS_MIN_GRID, the in-loop kernel: 81: odd row count, 52 r.r partials; 130 forced onto row-lds: 260
# tile partials, one reducing workgroup; 257: a second column block of ONE column; 513: last tile of one column, n^2 odd, 2565
# tile partials (slice 11 x 234 workgroups); 640: 3200 partials (slice 13 x 247)
SLAB_CASES = {
    "81": (81, "constant", None, "row-direct"),
    "130": (130, "constant", None, "row-direct"),
    "130-lds": (130, "random", "2", "row-lds"),
    "257": (257, "constant", None, "row-direct"),
    "513": (513, "random", None, "row-lds"),
    "640": (640, "constant", None, "row-lds"),
}
_cache = {}


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def coefficients(O, n, kind):
    """COO entries and CSR arrays: the constant stencil, or one random value per undirected edge (symmetric positive definite)"""
    key = ("matrix", n, kind)
    if key not in _cache:
        e = O.stencil5_coo(n) if kind == "constant" else symmetric_coo(O, n, np.random.default_rng(1000 + n))
        _cache[key] = (e,) + tuple(O.build_csr(e, n * n))
    return _cache[key]


def vectors(n, zero_x0=False):
    rng = np.random.default_rng(7 * n)
    b, x0 = rng.standard_normal(n * n), 0.1 * rng.standard_normal(n * n)
    return b, np.zeros(n * n) if zero_x0 else x0


def restated(O, n, kind, form, device_form=False, tol=TOL, zero_x0=False, ell=False):
    """The restated solve of one system: computed once, shared by every test that needs it."""
    key = ("solve", n, kind, form, device_form, tol, zero_x0, ell)
    if key not in _cache:
        _, rp, ci, va = coefficients(O, n, kind)
        system = CG.ellpack(O, rp, ci, va) if ell else CG.whole_grid(O, rp, ci, va, n, form, device_form)
        _cache[key] = CG.solve(system, *vectors(n, zero_x0), MAX_ITERS, tol)
    return _cache[key]


def check(got, want, what):
    """(x, history, iterations, converged), bit for bit"""
    x, h, it, conv = got
    wx, wh, wit, wconv = want
    assert (it, conv) == (wit, wconv), (what, it, conv, wit, wconv)
    assert len(h) == len(wh), what
    diff = np.flatnonzero(np.ascontiguousarray(h).view(np.uint64) != np.ascontiguousarray(wh).view(np.uint64))
    assert len(diff) == 0, (what, "history differs first at", int(diff[0]), float(h[diff[0]]), float(wh[diff[0]]))
    assert same_bits(x, wx), what


def slab_result(slab, st):
    return slab.gather(), slab.history(), st.iterations, st.converged


@pytest.mark.parametrize("case", list(SLAB_CASES))
def test_slab_solve_is_the_restated_solve(B, O, monkeypatch, case):
    n, kind, min_grid, form = SLAB_CASES[case]
    if min_grid is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", min_grid)
    e = coefficients(O, n, kind)[0]
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    try:
        assert slab.variant() == "stencil5/" + form
        slab.set_vectors(*vectors(n))
        st = slab.solve(max_iters=MAX_ITERS, tol=TOL)
        want = restated(O, n, kind, form)
        assert want[3] == 1 and want[2] > 10
        check(slab_result(slab, st), want, case)
    finally:
        slab.destroy()


@pytest.mark.parametrize("option,value", [("block_rows", 4), ("block_rows", 8), ("block_rows", 0), ("csr_coefficients", 1)])
def test_slab_solve_640_in_its_other_forms(Blab, O, option, value):
    """The block kernel (4 and 8 grid rows per wave), the one-row kernel and the CSR coefficient form at 640^2."""
    n = 640
    e = coefficients(O, n, "constant")[0]
    slab = Blab.CgSlab.from_matrix(Blab.HostMatrix(e, n * n, n * n, n))
    try:
        slab.set_option(option, value)
        assert slab.coefficient_form() == (0 if option == "csr_coefficients" else 1)
        slab.set_vectors(*vectors(n))
        st = slab.solve(max_iters=MAX_ITERS, tol=TOL)
        check(slab_result(slab, st), restated(O, n, "constant", "row-lds"), (option, value))
    finally:
        slab.destroy()
        Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.parametrize("mode,n,form", [("stencil5-csr", 130, "row-direct"), ("stencil5-csr", 640, "row-lds"), ("ellpack", 130, None)])
def test_cg_solve_device_is_the_restated_solve(B, O, mode, n, form):
    """cg_solve_device: the same loop with the single-GPU direction rounding fma(beta, p, r). stencil5-csr takes its SpMV's fused
    p.Ap (and, on row-lds, the fused initial residual); the ELLPACK operator's fused p.Ap is ell_block_dot's."""
    e = coefficients(O, n, "constant")[0]
    m = B.HostMatrix(e, n * n, n * n, n)
    op = B.Operator(mode)
    assert op.init(m) == 0
    B.lib().spmv_amd_cg_release_workspace()
    try:
        if form is not None:
            assert op.variant() == "stencil5/" + form
        b, x0 = vectors(n)
        x, hist, st = B.cg_solve(op, m, b, x0, max_iters=MAX_ITERS, tol=TOL, device=True)
        check((x, hist, st.iterations, st.converged), restated(O, n, "constant", form, device_form=True, ell=form is None), (mode, n))
    finally:
        op.free()


@pytest.mark.parametrize("as_rank,as_world", [(0, 2), (1, 4)])
def test_stand_in_slab_with_extras_is_the_restated_solve(Blab, O, monkeypatch, as_rank, as_world):
    """A slab with neighbours: its boundary rows' tile partials enter the second stage as extras -- of the reducing launch that
    also evaluates them in the loop, of the plain reduction for r0 -- behind the slice sums of the interior rows' partials. Nine
    iterations, tolerance 0, pipeline and plain order; the all-reduces run over the one rank and hand the local sum back."""
    monkeypatch.setenv("SPMV_AMD_SELF_NEIGHBOUR", "1")
    monkeypatch.setenv("SPMV_AMD_FORCE_COLLECTIVES", "1")
    n, iterations = 1024, 9
    system, off, nl = CG.stand_in(O, n, as_rank, as_world)
    rng = np.random.default_rng(as_world)
    b, x0 = rng.standard_normal(n * n), 0.1 * rng.standard_normal(n * n)
    want = CG.solve(system, b[off:off + nl], x0[off:off + nl], iterations, 0.0)
    assert want[2:] == (iterations, 0)
    comm = Blab.Comm.rccl(0, 1, Blab.Comm.unique_id())
    assert comm is not None and comm.transport() == "rccl"
    slab = Blab.CgSlab.stencil5_as(n, as_rank, as_world, comm)
    try:
        assert (slab.row_offset, slab.n_local) == (off, nl) and slab.variant() == "stencil5/row-lds"
        slab.set_vectors(b, x0)
        shapes = set()
        for no_overlap in (0, 1):
            slab.set_option("no_overlap", no_overlap)
            st = slab.solve(max_iters=iterations, tol=0.0)
            shapes.add(slab.loop_shape().split(":")[0].split(" ")[0])
            got = (slab.gather()[:nl], slab.history(), st.iterations, st.converged)  # one rank: the slab's x lies at the front
            check(got, want, (as_rank, as_world, no_overlap, slab.loop_shape()))
        assert shapes == {"pipeline", "plain"}, shapes
    finally:
        slab.destroy()
        comm.destroy()


# ---------------------------------------------------------------- the stopping test at its boundary
def boundary(h):
    """k = the first index whose ratio to h[0] is below 1e-4, asserted to be the first, and that ratio as the device forms it."""
    ratio = h / h[0]  # one IEEE division per entry
    k = int(np.flatnonzero(ratio < 1e-4)[0])
    assert k > 2 and np.all(ratio[:k] >= 1e-4) and ratio[k] < 1e-4
    return k, float(ratio[k])


def check_boundary(O, solve, n, device_form, form, what):
    """solve(tol) -> (x, history, iterations, converged) on the constant n x n stencil, random b, x0 = 0."""
    h = solve(1e-6)[1]
    long_run = restated(O, n, "constant", form, device_form=device_form, tol=1e-6, zero_x0=True)
    assert same_bits(h, long_run[1]), what
    k, t = boundary(h)
    # tol == the ratio itself: the comparison is strict, iteration k goes on
    x, hist, it, conv = solve(t)
    assert it > k and same_bits(hist[:k + 1], h[:k + 1]), (what, it, k)
    # the next double: stops at exactly k
    above = float(np.nextafter(t, np.inf))
    got = solve(above)
    want = restated(O, n, "constant", form, device_form=device_form, tol=above, zero_x0=True)
    assert want[2:] == (k, 1) and same_bits(want[1], h[:k + 1])
    check(got, want, what)


@pytest.mark.parametrize("ring", ["1", "16"])
@pytest.mark.parametrize("n,form", [(130, "row-direct"), (640, "row-lds")])
def test_slab_stopping_test_at_its_boundary(Blab, O, monkeypatch, n, form, ring):
    """Every run-ahead rule of the host (0: every record awaited; 1: the 16 x rule; 2: always one iteration ahead, so the
    converging iteration is found late and an empty iteration is enqueued behind it) and both settings of the overlap switch."""
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    e = coefficients(O, n, "constant")[0]
    slab = Blab.CgSlab.from_matrix(Blab.HostMatrix(e, n * n, n * n, n))
    try:
        assert slab.variant() == "stencil5/" + form
        slab.set_vectors(*vectors(n, zero_x0=True))

        def solve(tol):
            st = slab.solve(max_iters=MAX_ITERS, tol=tol)
            return slab_result(slab, st)

        for run_ahead in (0, 1, 2):
            for no_overlap in (0, 1):
                slab.set_option("run_ahead", run_ahead)
                slab.set_option("no_overlap", no_overlap)
                check_boundary(O, solve, n, False, form, (n, ring, run_ahead, no_overlap))
    finally:
        slab.destroy()
        Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.parametrize("ring", ["1", "16"])
@pytest.mark.parametrize("n,form", [(130, "row-direct"), (640, "row-lds")])
def test_cg_solve_device_stopping_test_at_its_boundary(B, O, monkeypatch, n, form, ring):
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    e = coefficients(O, n, "constant")[0]
    m = B.HostMatrix(e, n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    B.lib().spmv_amd_cg_release_workspace()  # the workspace, and with it the direction ring, is created by the next solve
    try:
        assert op.variant() == "stencil5/" + form
        b, x0 = vectors(n, zero_x0=True)

        def solve(tol):
            x, hist, st = B.cg_solve(op, m, b, x0, max_iters=MAX_ITERS, tol=tol, device=True)
            return x, hist, st.iterations, st.converged

        check_boundary(O, solve, n, True, form, (n, ring))
    finally:
        op.free()
