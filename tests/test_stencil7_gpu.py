"""The "stencil7-csr" operator (n x n x n 7-point stencil) on the GPU. Its contract makes oracle.spmv_csr -- the sequential CSR
loop, sum from +0.0 in ascending column order -- the bit-for-bit oracle of every row in every variant, so everything here is an
equality of arrays or of bit patterns: the SpMV kernels at the sizes where each can go wrong, signed zeros and non-finite
isolation, the device generator, recognition of what is not a 3-D stencil, whole CG solves against the restated loop
(tests/cg_restatement.py with rowlds_partials / rowdirect_partials over n^2 grid rows), and the solvers that come with an
operator of this library (Jacobi, Chebyshev, SpMM, the multigrid refusal, lifecycle)."""
import numpy as np
import pytest

import cg_restatement as CG
import csr_restatement as CR
import matrices as M
import reduction_restatement as R
import stencil7 as S7
from bitwise import same_bits
from conftest import hist_err

pytestmark = pytest.mark.gpu

VARIANTS = (None, "row-lds", "row-direct")
_cache = {}


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_operator_select_variant(b"stencil7-csr", None)
    B.lib().spmv_amd_reset_host_matrices()


class Shift:  # view one double into the allocation: 8-byte-only aligned vectors
    def __init__(self, v):
        self.ptr = v.ptr + 8


def init(B, op, m):
    """init from a host matrix; build_csr_struct re-uses csr_mat when (rows, nnz) match, so start from a clean slate"""
    B.lib().spmv_amd_reset_host_matrices()
    assert op.init(m) == 0


def random_system(O, n):
    """random coefficients in every entry (unsymmetric), x ~ N(0, 1), the CSR and the oracle's y: built once per n"""
    if n not in _cache:
        rng = np.random.default_rng(700 + n)
        e = S7.coo(n, rng=rng)
        x = rng.standard_normal(n ** 3)
        rp, ci, va = O.build_csr(e, n ** 3)
        _cache[n] = (e, x, rp, ci, va, O.spmv_csr(rp, ci, va, x))
    return _cache[n]


def auto_name(n):
    return "stencil7/row-lds" if n >= 64 else "stencil7/row-direct"


def check_both_entry_points(B, op, x, want, what):
    got, ms = op.run_timed(x)
    assert ms > 0 and np.array_equal(got, want), what
    N = len(x)
    dx, dy = B.DeviceVector.from_host(x), B.DeviceVector(N, fill=-7.0)
    sx, sy = B.DeviceVector.from_host(np.concatenate([[0.0], x])), B.DeviceVector(N + 1, fill=-7.0)
    try:
        assert op.run_device(dx, dy) == 0
        assert np.array_equal(dy.to_host(), want), what
        assert op.run_device(Shift(sx), Shift(sy)) == 0
        out = sy.to_host()
        assert np.array_equal(out[1:], want) and out[0] == -7.0, what
    finally:
        for v in (dx, dy, sx, sy):
            v.free()


# 2: no interior grid row; 3: exactly one; 4, 5: the tile's second half dead; 65: one live column in it; 128: a full tile whose
# lane 63 ends the grid row; 129, 130: a last tile of one / two columns
@pytest.mark.parametrize("n", [2, 3, 4, 5, 65, 128, 129, 130])
def test_spmv_bit_for_bit(B, O, monkeypatch, n):
    e, x, rp, ci, va, want = random_system(O, n)
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    try:
        for forced in VARIANTS:
            assert op.select_variant(forced) == 0
            assert op.variant() == (auto_name(n) if forced is None else "stencil7/" + forced)
            check_both_entry_points(B, op, x, want, (n, forced))
        if n == 130:
            # an XCD run that does not divide the tile count (130^2 * 2 tiles): the padded grid's surplus workgroups do nothing
            monkeypatch.setenv("SPMV_AMD_ROWLDS_GROUP", "3")
            assert op.select_variant("row-lds") == 0
            check_both_entry_points(B, op, x, want, (n, "run 3"))
    finally:
        op.select_variant(None)
        op.free()


@pytest.mark.parametrize("n", [6, 65])
def test_signed_zeros_and_non_finite_isolation(B, O, n):
    rng = np.random.default_rng(n)
    N = n ** 3
    e = S7.coo(n, rng=rng)
    e["value"] = np.abs(e["value"]) + 0.5  # positive: a product with -0.0 is -0.0
    rp, ci, va = O.build_csr(e, N)
    # planes 1..3 of x hold -0.0: every product of every row of plane 2 is -0.0, and the loop's sum from +0.0 is +0.0
    xz = rng.standard_normal(N)
    xz[n * n:4 * n * n] = -0.0
    wz = O.spmv_csr(rp, ci, va, xz)
    assert not np.signbit(wz[2 * n * n:3 * n * n]).any() and (wz[2 * n * n:3 * n * n] == 0.0).all()
    # x[0] = inf: only rows 0, 1, n and n^2 hold column 0; no lane of a dead column or an absent neighbour multiplies it
    xi = rng.standard_normal(N)
    xi[0] = np.inf
    wi = O.spmv_csr(rp, ci, va, xi)
    touched = np.zeros(N, dtype=bool)
    touched[[0, 1, n, n * n]] = True
    assert np.isfinite(wi[~touched]).all() and np.isinf(wi[touched]).all()
    # the same on the fast path: inf in column n - 1 of an interior grid row (n = 65: the one live column of the tile's second half,
    # beside 63 dead lanes, the zero-filled strip and x slots and the LDS W / E copy); only the rows that hold that column see it
    xf = rng.standard_normal(N)
    hot = 2 * n * n + 2 * n + (n - 1)
    xf[hot] = np.inf
    wf = O.spmv_csr(rp, ci, va, xf)
    seen = np.zeros(N, dtype=bool)
    seen[np.repeat(np.arange(N), np.diff(rp))[ci == hot]] = True
    assert seen.sum() == 6 and np.isfinite(wf[~seen]).all() and np.isinf(wf[seen]).all()
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, N, N, n))
    try:
        for forced in ("row-lds", "row-direct"):
            assert op.select_variant(forced) == 0 and op.variant() == "stencil7/" + forced
            for x, want in ((xz, wz), (xi, wi), (xf, wf)):
                got, _ = op.run_timed(x)
                assert same_bits(got, want), (n, forced)
    finally:
        op.select_variant(None)
        op.free()


@pytest.mark.parametrize("n", [1, 2, 3, 9, 64])
def test_generator_equals_the_host_path(B, O, n):
    N = n ** 3
    rp, ci, va = O.build_csr(S7.coo(n), N)
    x = np.random.default_rng(n).standard_normal(N)
    want = O.spmv_csr(rp, ci, va, x)
    ys = {}
    for mode in ("stencil7-csr", "cusparse-csr"):
        op = B.Operator(mode)
        assert op.init_synthetic3d(n) == 0
        try:
            if mode == "stencil7-csr":
                assert op.variant() == ("stencil7/csr-loop" if n == 1 else auto_name(n))
            grp, gci, gva = op.download_csr(N, S7.nnz(n))
            assert np.array_equal(grp, rp) and np.array_equal(gci, ci) and np.array_equal(gva, va), mode
            ys[mode], _ = op.run_timed(x)
        finally:
            op.free()
    assert np.array_equal(ys["stencil7-csr"], want) and np.array_equal(ys["cusparse-csr"], want)


def test_generator_256_checksum(B):
    """16.7 M rows generated on the device: y = A 1 holds small integers, so the sum is exact whatever its order"""
    n = 256
    N = n ** 3
    op = B.Operator("stencil7-csr")
    assert op.init_synthetic3d(n) == 0
    dx, dy = B.DeviceVector(N, fill=1.0), B.DeviceVector(N, fill=-7.0)
    try:
        assert op.variant() == "stencil7/row-lds"
        assert op.run_device(dx, dy) == 0
        y = dy.to_host()
        assert y.sum() == N + 6 * n * n and y.min() == 1.0 and y.max() == 4.0
    finally:
        dx.free(), dy.free(), op.free()


def _not_a_3d_stencil(O):
    """name -> (entries, rows, grid_size): matrices "stencil7-csr" must run through the CSR loop"""
    n = 6
    N = n ** 3
    rng = np.random.default_rng(66)
    good = S7.coo(n, rng=rng)
    moved = good.copy()
    r = 2 * n * n + 2 * n + 2  # an interior point: its E entry goes to column r + 2, which the pattern does not hold
    k = int(np.flatnonzero((moved["row"] == r) & (moved["col"] == r + 1))[0])
    moved["col"][k] = r + 2
    shortened = np.delete(good, k)
    other_row = good.copy()  # the same entry handed to row r + 3: nnz is right, two row lengths are not
    other_row["row"][k] = r + 3
    nine, rows9, _, _ = M.stencil_9point(8)  # 64 rows = 4^3
    five, rows5, _ = M.stencil_random_values(8)
    return {"one entry moved": (moved, N, n), "entry in another row": (other_row, N, n), "one row shortened": (shortened, N, n), "9-point as 4^3": (nine, rows9, 4),
            "no grid size": (good, N, -1), "2-D 5-point, grid 8": (five, rows5, 8), "2-D 5-point, grid 4": (five, rows5, 4)}


@pytest.mark.parametrize("case", ["one entry moved", "entry in another row", "one row shortened", "9-point as 4^3", "no grid size", "2-D 5-point, grid 8",
                                  "2-D 5-point, grid 4"])
def test_what_is_not_a_3d_stencil_takes_the_csr_loop(B, O, case):
    e, rows, grid = _not_a_3d_stencil(O)[case]
    rp, ci, va = O.build_csr(e, rows)
    x = np.random.default_rng(5).standard_normal(rows)
    want = O.spmv_csr(rp, ci, va, x)
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, rows, rows, grid))
    try:
        for forced in (None, "row-lds", "row-direct", "csr-loop"):
            assert op.select_variant(forced) == 0
            assert op.variant() == "stencil7/csr-loop", (case, forced)
            got, _ = op.run_timed(x)
            assert np.array_equal(got, want), (case, forced)
    finally:
        op.select_variant(None)
        op.free()


@pytest.mark.parametrize("mode", ["stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"])
def test_the_other_operators_are_not_fooled_by_the_grid_size(B, O, mode):
    """a 3-D matrix carries grid_size = n and n^3 rows: no 2-D fast path may take it"""
    n = 6
    e, x, rp, ci, va, want = random_system(O, n)
    op = B.Operator(mode)
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    try:
        got, _ = op.run_timed(x)
        tree = op.variant() in ("csr/wavefront", "csr/adaptive")  # the variants whose sum is a tree: the existing scaled bound
        assert np.array_equal(got, want) or (tree and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))), op.variant()
        if tree:  # ... and the bits of the kernel's own order
            assert same_bits(got, CR.row_sums(rp, ci, va, x, CR.variant_of(rp, op.variant()))), op.variant()
        assert "stencil5-direct" not in op.variant() and op.variant() not in ("stencil5/row-lds", "stencil5/row-direct")
    finally:
        op.free()


def test_forced_csr_loop_on_a_verified_matrix(B, O):
    n = 9
    e, x, rp, ci, va, want = random_system(O, n)
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    try:
        assert op.select_variant("csr-loop") == 0 and op.variant() == "stencil7/csr-loop"
        check_both_entry_points(B, op, x, want, "csr-loop")
    finally:
        op.select_variant(None)
        op.free()


# ---------------------------------------------------------------- dot partials through whole solves
TOL, MAX_ITERS = 1e-8, 500
PARTIALS = {"row-lds": R.rowlds_partials, "row-direct": R.rowdirect_partials}


def cg_system(O, n, center):
    key = ("cg", n, center)
    if key not in _cache:
        e = S7.coo(n, center=center, off=-1.0)
        rng = np.random.default_rng(31 * n + int(center))
        _cache[key] = (e,) + tuple(O.build_csr(e, n ** 3)) + (rng.standard_normal(n ** 3), rng.standard_normal(n ** 3))
    return _cache[key]


def restated(O, n, center, form):
    key = ("restated", n, center, form)
    if key not in _cache:
        e, rp, ci, va, b, x0 = cg_system(O, n, center)
        system = CG.System(spmv=lambda v: O.spmv_csr(rp, ci, va, v), pap=lambda p, ap: (PARTIALS[form](p, ap, n), ()), rr0=CG.stream_rr0,
                           device_form=True)
        _cache[key] = CG.solve(system, b, x0, MAX_ITERS, TOL)
    return _cache[key]


@pytest.mark.parametrize("form", ["row-lds", "row-direct"])
@pytest.mark.parametrize("center", [7.0, 6.0])
@pytest.mark.parametrize("n", [20, 33])
def test_cg_solve_device_is_the_restated_solve(B, O, n, center, form):
    """cg_solve_device around stencil7-csr: the fused p.Ap partials in the kernels' own shapes, the streaming initial residual,
    the device form's direction update: iteration count, verdict, every history entry and x, bit for bit"""
    e, rp, ci, va, b, x0 = cg_system(O, n, center)
    m = B.HostMatrix(e, n ** 3, n ** 3, n)
    op = B.Operator("stencil7-csr")
    init(B, op, m)
    B.lib().spmv_amd_cg_release_workspace()
    try:
        assert op.select_variant(form) == 0 and op.variant() == "stencil7/" + form
        x, hist, st = B.cg_solve(op, m, b, x0, max_iters=MAX_ITERS, tol=TOL, device=True)
        wx, wh, wit, wconv = restated(O, n, center, form)
        assert wconv == 1 and wit > 10
        assert (st.iterations, st.converged) == (wit, wconv), (st.iterations, st.converged, wit, wconv)
        assert len(hist) == len(wh)
        diff = np.flatnonzero(np.ascontiguousarray(hist).view(np.uint64) != np.ascontiguousarray(wh).view(np.uint64))
        assert len(diff) == 0, ("history differs first at", int(diff[0]), float(hist[diff[0]]), float(wh[diff[0]]))
        assert same_bits(x, wx)
    finally:
        op.select_variant(None)
        op.free()


# ---------------------------------------------------------------- the solvers on top
def test_jacobi_inverse_diagonal(B, O):
    n = 9
    N = n ** 3
    rng = np.random.default_rng(9)
    e = S7.coo(n, rng=rng)
    d = rng.uniform(1.0, 9.0, N)
    diag = e["row"] == e["col"]
    e["value"][diag] = d[e["row"][diag]]
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, N, N, n))
    pc = B.Precond(op, "jacobi")
    try:
        assert same_bits(pc.inverse_diagonal(), 1.0 / d)
    finally:
        pc.destroy()
        op.free()


def test_jacobi_and_chebyshev_pcg_agree_with_the_csr_operator(B, O):
    n = 16
    N = n ** 3
    rng = np.random.default_rng(16)
    e = S7.spd_coo(n, rng)
    b = rng.standard_normal(N)
    m = B.HostMatrix(e, N, N, n)
    runs = {}
    for mode in ("stencil7-csr", "cusparse-csr"):
        op = B.Operator(mode)
        init(B, op, m)
        try:
            if mode == "stencil7-csr":
                assert op.variant() == "stencil7/row-direct"
            for kind in ("jacobi", "chebyshev"):
                pc = B.Precond(op, "jacobi") if kind == "jacobi" else B.Precond.chebyshev(op, degree=4)
                try:
                    x, hist, st = B.pcg_solve_device(op, m, pc, b, np.zeros(N), max_iters=500, tol=1e-8)
                    info = pc.chebyshev_info() if kind == "chebyshev" else None
                    runs[mode, kind] = (x, hist, st.iterations, st.converged, None if info is None else info[2])
                finally:
                    pc.destroy()
        finally:
            op.free()
    for kind in ("jacobi", "chebyshev"):
        x7, h7, it7, conv7, lmax7 = runs["stencil7-csr", kind]
        xc, hc, itc, convc, lmaxc = runs["cusparse-csr", kind]
        assert conv7 == convc == 1 and it7 == itc and len(h7) == len(hc), (kind, it7, itc)
        assert hist_err(h7, hc) < 1e-10, kind  # the project's CG parity bound, per entry
        if kind == "chebyshev":
            assert same_bits([lmax7], [lmaxc])


@pytest.mark.parametrize("k", [1, 3, 8])
def test_spmm_columns_are_run_device(B, O, k):
    n = 9
    e, x, rp, ci, va, want = random_system(O, n)
    N = n ** 3
    X = np.random.default_rng(k).standard_normal((k, N))
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, N, N, n))
    dy = B.DeviceVector(N, fill=-7.0)
    try:
        Y = op.run_spmm(X)
        for j in range(k):
            dx = B.DeviceVector.from_host(X[j])
            assert op.run_device(dx, dy) == 0
            assert same_bits(Y[j], dy.to_host()), (k, j)
            assert np.array_equal(Y[j], O.spmv_csr(rp, ci, va, X[j]))
            dx.free()
    finally:
        dy.free()
        op.free()


def test_multigrid_is_refused_and_leaves_nothing(B, O):
    n = 9
    e = S7.coo(n)
    op = B.Operator("stencil7-csr")
    init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
    try:
        before = B._multi_lib().spmv_amd_cg_multi_workspace_bytes()
        with pytest.raises(ValueError):
            B.Precond.multigrid(op)
        assert B._multi_lib().spmv_amd_cg_multi_workspace_bytes() == before
        got, _ = op.run_timed(np.ones(n ** 3))  # the operator is untouched
        assert got.sum() == n ** 3 + 6 * n * n
    finally:
        op.free()


def test_lifecycle(B, O):
    op = B.Operator("stencil7-csr")
    for n in (5, 7):  # init -> free -> init at another size
        e, x, rp, ci, va, want = random_system(O, n)
        init(B, op, B.HostMatrix(e, n ** 3, n ** 3, n))
        assert np.array_equal(op.run_timed(x)[0], want)
        op.free()
        assert op.variant() == "uninitialised"
    assert op.init_synthetic3d(4) == 0  # from host after synthetic, without a free in between
    n = 5
    e = S7.spd_coo(n, np.random.default_rng(55))
    N = n ** 3
    rp, ci, va = O.build_csr(e, N)
    m = B.HostMatrix(e, N, N, n)
    init(B, op, m)
    x = np.random.default_rng(56).standard_normal(N)
    assert np.array_equal(op.run_timed(x)[0], O.spmv_csr(rp, ci, va, x))
    # a preconditioner from before a re-init is refused (generation counter)
    b = np.ones(N)
    stale = B.Precond(op, "jacobi")
    x1, h1, _ = B.pcg_solve_device(op, m, stale, b, np.zeros(N))
    init(B, op, m)
    with pytest.raises(RuntimeError):
        B.pcg_solve_device(op, m, stale, b, np.zeros(N))
    fresh = B.Precond(op, "jacobi")
    x2, h2, _ = B.pcg_solve_device(op, m, fresh, b, np.zeros(N))
    assert np.array_equal(x2, x1) and np.array_equal(h2, h1)
    stale.destroy(), fresh.destroy()
    op.free()
