"""Poisoned inputs on the GPU: each stencil kernel reads only what its rows hold (the AMG transfers and the CSR family: the "general CSR"
section of tests/poison.py, run by tests/test_poison_csr_gpu.py). Every test runs a kernel family on a poisoned system
of tests/poison.py -- +inf in x at the seam positions of the 128-column tile, -0.0 over a whole neighbourhood, +inf in stored
coefficients (the first and last entry of the matrix, where every clamped coefficient run lands, among them) -- and compares with the
oracle through same_bits_nan_as_class: a value that is read and then cancelled (multiplied by 0.0, added to a sum) shows as a
non-finite row the oracle does not have, or as a zero of the wrong sign. tests/test_poison_host.py shows that the oracle's own
non-finite rows are exactly the matrix's adjacency of the poison, so no adjacency logic runs here. Caller-owned vectors sit between
sentinels, outputs start as NaN, inputs keep their bits. No whole solve is run on poisoned data. Every system comes from
tests/poison.py, where the host file holds it; what a stage cannot take (the CSR form has no launch that reads the planes, a matrix
with an inf coefficient does not let b stand for r0, a slab with a mixed row block does not recompute A p) is asserted as a refusal."""
import functools

import numpy as np
import pytest

import chebyshev_restatement as CR
import multigrid3d_restatement as M3
import multigrid_restatement as MG
import poison as P
import reduction_restatement as RR
import tile_classes as T
from bitwise import same_bits, same_bits_nan_as_class
from test_chebyshev_gpu import Guarded
from test_mg_multi_stages_gpu import Shifted, column, interleaved
from test_multigrid_gpu import GuardedBytes

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 8)
ODD_2D = (9, 129, 257)  # the transfer kernels' grids: odd, so the lone last row and column take part
ODD_3D = (65, 129)


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def host_matrix(B, s):
    rows = s.n ** s.dim
    return B.HostMatrix(P.entries_of(s.rp, s.ci, s.va), rows, rows, s.n)


def run_between_sentinels(B, op, x, want, what):
    """run_device on x between sentinels and y started as NaN, 16-byte aligned and 8 bytes off: y is the oracle's, x keeps its bits."""
    for shift in (0, 1):
        hold = (lambda v: Shifted(B, v, shift)) if shift else (lambda v: Guarded(B, v))
        dx, dy = hold(x), hold(np.full(len(want), np.nan))
        try:
            assert op.run_device(dx, dy) == 0
            assert same_bits_nan_as_class(dy.read(), want), what
            assert same_bits(dx.read(), x), what
        finally:
            dx.free(), dy.free()


# ---------------------------------------------------------------- the single-vector operators
@pytest.mark.parametrize("planter", P.PLANTERS)
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_stencil5_csr_variants(B, O, monkeypatch, n, planter):
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "2")
    s = P.system(n, planter)
    want = O.spmv_stencil5(s.rp, s.ci, s.va, s.x, n)
    op = B.Operator("stencil5-csr")
    assert op.init(host_matrix(B, s)) == 0
    try:
        assert op.variant() == "stencil5/row-lds"
        for forced in ("row-lds", "row-direct", "row-generic"):
            assert op.select_variant(forced) == 0 and op.variant() == "stencil5/" + forced
            run_between_sentinels(B, op, s.x, want, (n, planter, forced))
            got, _ = op.run_timed(s.x)
            assert same_bits_nan_as_class(got, want), (n, planter, forced)
    finally:
        op.select_variant(None)
        op.free()


@pytest.mark.parametrize("planter", P.PLANTERS)
@pytest.mark.parametrize("n", P.GRIDS_2D)
@pytest.mark.parametrize("name", ["stencil5-ellpack", "ellpack"])
def test_ellpack_operators(B, O, name, n, planter):
    s = P.system(n, planter, 2, False)  # coef_inf: the seam entries, without the first and last entry of the matrix
    want = O.spmv_stencil5(s.rp, s.ci, s.va, s.x, n) if name == "stencil5-ellpack" else O.spmv_csr(s.rp, s.ci, s.va, s.x)
    op = B.Operator(name)
    assert op.init(host_matrix(B, s)) == 0
    try:
        assert op.variant() == ("ell/stencil5-direct" if name == "stencil5-ellpack" else "ell/slot-major")
        run_between_sentinels(B, op, s.x, want, (name, n, planter))
    finally:
        op.free()


@pytest.mark.parametrize("name", ["stencil5-ellpack", "ellpack"])
def test_ellpack_padding_reaches_no_column(B, O, name):
    """Ragged rows, none with an entry in column 0 or in the last column: +inf there can only be reached through a padding slot."""
    e, r, c, x = P.padding_case()
    rp, ci, va = O.build_csr(e, r)
    want = O.spmv_csr(rp, ci, va, x)
    assert np.isfinite(want).all()
    op = B.Operator(name)
    assert op.init(B.HostMatrix(e, r, c, -1)) == 0
    try:
        assert op.variant() == "ell/slot-major"
        run_between_sentinels(B, op, x, want, name)
    finally:
        op.free()


@pytest.mark.parametrize("variant", ["stream", "row-scalar"])
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_csr_operator_sequential_variants(B, O, n, variant):
    """The second witness: the sequential CSR kernels on the stencil matrix with +inf in x."""
    s = P.system(n, "x_inf")
    want = O.spmv_csr(s.rp, s.ci, s.va, s.x)
    op = B.Operator("cusparse-csr")
    op.select_variant(variant)
    try:
        assert op.init(host_matrix(B, s)) == 0 and op.variant() == "csr/" + variant
        run_between_sentinels(B, op, s.x, want, (n, variant))
    finally:
        op.free()
        op.select_variant(None)


@pytest.mark.parametrize("n", P.GRIDS_3D)
def test_stencil7_csr_poisoned_coefficients(B, O, n):
    s = P.system(n, "coef_inf", 3)
    want = O.spmv_csr(s.rp, s.ci, s.va, s.x)
    op = B.Operator("stencil7-csr")
    assert op.init(host_matrix(B, s)) == 0
    try:
        for forced in ("row-lds", "row-direct"):
            assert op.select_variant(forced) == 0 and op.variant() == "stencil7/" + forced
            run_between_sentinels(B, op, s.x, want, (n, forced))
    finally:
        op.select_variant(None)
        op.free()


# ---------------------------------------------------------------- the fused Chebyshev step
@pytest.mark.parametrize("case", P.CHEBYSHEV_CASES)
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_fused_chebyshev_step(B, O, monkeypatch, n, case):
    """The fused step of the row-lds plan (the tile's product, then d and z updated in the same launch) through an application
    z = M^-1 r on the caller's r between sentinels, degrees 1 and 2, against chebyshev_restatement.make_apply with the library's
    own coefficients. The stage hook has no kind for this step, so its inputs cannot be poisoned one at a time; the three cases
    of poison.chebyshev_system reach all four: +inf in r is +inf in z and d at the same places when the first step runs, a
    subnormal diagonal is +inf in dinv (r finite), and an inf off-diagonal coefficient meets finite vectors. The unfused step of
    the row-direct variant must give the same."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "2")
    s = P.chebyshev_system(n, case)
    rows, r = n * n, s.x
    with np.errstate(over="ignore"):
        dinv = 1.0 / s.va[P.row_of_entry(s.rp) == s.ci]
    matvec = lambda v: O.spmv_stencil5(s.rp, s.ci, s.va, v, n)
    op = B.Operator("stencil5-csr")
    assert op.init(host_matrix(B, s)) == 0
    dr = Guarded(B, r)
    try:
        for forced in ("row-lds", "row-direct"):
            assert op.select_variant(forced) == 0 and op.variant() == "stencil5/" + forced
            for degree in (1, 2):
                pc = B.Precond.chebyshev(op, degree, *P.CHEBYSHEV_BOUNDS)
                dz = Guarded(B, np.full(rows, np.nan))
                try:
                    coef = pc.chebyshev_info()[3]
                    assert same_bits(pc.inverse_diagonal(), dinv), (n, case)
                    with np.errstate(invalid="ignore", over="ignore"):
                        want = CR.make_apply(matvec, dinv, list(coef), fma=O.axpy)(r)
                    assert not np.isfinite(want).all() and (n == 9 or 2 * np.isfinite(want).sum() > rows)
                    pc.apply_device(op, dr.ptr, dz.ptr)
                    assert same_bits_nan_as_class(dz.read(), want), (n, case, forced, degree)
                    assert same_bits(dr.read(), r), (n, case, forced, degree)
                finally:
                    dz.free()
                    pc.destroy()
    finally:
        dr.free()
        op.select_variant(None)
        op.free()


# ---------------------------------------------------------------- the block product of the 2-D operator
@functools.lru_cache(maxsize=None)
def clean_columns(n, dim=2):
    """Eight finite columns for the blocks: the poisoned x of a system replaces one of them."""
    X = np.random.default_rng(4000 + 10 * n + dim).standard_normal((8, n ** dim))
    X.setflags(write=False)
    return X


def block_of(s, k):
    """k columns, the system's x (poisoned for the x planters) in column k // 2 only."""
    X = clean_columns(s.n, s.dim)[:k].copy()
    X[k // 2] = s.x
    return X


@pytest.mark.parametrize("planter", P.PLANTERS)
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_run_spmm_rows_and_columns(B, O, monkeypatch, n, planter):
    """Row isolation as in the single-vector product, and column isolation: the poison sits in one column of the block, the others
    come out bit-equal to their own product (under coef_inf every column sees the matrix's poison, each as the oracle does)."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "2")
    s = P.system(n, planter)
    rows = n * n
    wants = {}

    def want(k, j):
        key = "x" if j == k // 2 else j
        if key not in wants:
            wants[key] = O.spmv_stencil5(s.rp, s.ci, s.va, s.x if key == "x" else clean_columns(n)[j], n)
        return wants[key]

    op = B.Operator("stencil5-csr")
    assert op.init(host_matrix(B, s)) == 0
    multi = B._multi_lib()
    try:
        for forced in ("row-lds", "row-direct", "row-generic"):
            assert op.select_variant(forced) == 0
            for k in KS:
                X = block_of(s, k)
                for shift in ((0, 1) if k % 2 == 1 else (0,)):
                    hold = (lambda v: Shifted(B, v, shift)) if shift else (lambda v: Guarded(B, v))
                    xb = interleaved(X, k)
                    dx, dy = hold(xb), hold(np.full(rows * k, np.nan))
                    try:
                        assert multi.spmv_amd_spmm_device(b"stencil5-csr", k, dx.ptr, dy.ptr) == 0
                        assert op.spmm_variant() == "spmm/stencil5-" + forced
                        got = dy.read()
                        for j in range(k):
                            gj, wj = column(got, k, j), want(k, j)
                            assert same_bits_nan_as_class(gj, wj), (n, planter, forced, k, j, shift)
                            if planter != "coef_inf" and j != k // 2:
                                assert np.isfinite(wj).all() and same_bits(gj, wj), (n, planter, forced, k, j, shift)
                        assert same_bits(dx.read(), xb)
                    finally:
                        dx.free(), dy.free()
    finally:
        op.select_variant(None)
        op.free()


# ---------------------------------------------------------------- multigrid transfers
@functools.lru_cache(maxsize=2)
def transfer_cases(n, dim):
    """rp, ci and (label, va, z, r, r_c) with +inf in z, in r and in a coefficient at the seam positions, and the restatement's
    r_c = restrict(r - A z) of each. n is odd: the lone last row, column (and plane) are among the positions."""
    from oracle import oracle as O

    R = MG if dim == 2 else M3
    si, sc = P.system(n, "x_inf_pairs", dim), P.system(n, "coef_inf", dim)
    clean = clean_columns(n, dim)
    product = (lambda va, v: O.spmv_stencil5(si.rp, si.ci, va, v, n)) if dim == 2 else (lambda va, v: O.spmv_csr(si.rp, si.ci, va, v))
    out = []
    # the +inf of z and r meets positive coefficients only: every poisoned residual is -inf (z) or +inf (r), the sum over an aggregate
    # never inf - inf, so a NaN a kernel makes of a cancelled neighbour cannot hide behind a NaN of the oracle's own
    positive = np.abs(si.va)
    for label, va, z, r in (("z", positive, si.x, clean[0]), ("r", positive, clean[1], si.x), ("coefficient", sc.va, sc.x, clean[2])):
        with np.errstate(invalid="ignore"):  # inf - inf inside an aggregate with two poisoned members
            out.append((label, va, z, r, R.restrict(O.axpy(-1.0, product(va, z), r), n)))
        assert label == "coefficient" or (np.isinf(out[-1][4]).any() and not np.isnan(out[-1][4]).any())
    return si.rp, si.ci, out


@functools.lru_cache(maxsize=64)
def clean_coarse_residual(n, dim, poisoned_matrix, j):
    """restrict(r - A z) of the finite columns j of the blocks (z = clean[j], r = clean[7 - j]): shared by every k."""
    from oracle import oracle as O

    s = P.system(n, "coef_inf" if poisoned_matrix else "x_inf_pairs", dim)
    clean = clean_columns(n, dim)
    va = s.va if poisoned_matrix else np.abs(s.va)
    az = O.spmv_stencil5(s.rp, s.ci, va, clean[j], n) if dim == 2 else O.spmv_csr(s.rp, s.ci, va, clean[j])
    with np.errstate(invalid="ignore"):  # a poisoned matrix: +inf and -inf may meet in one aggregate
        return (MG if dim == 2 else M3).restrict(O.axpy(-1.0, az, clean[7 - j]), n)


def coarse_poison(n, dim):
    """A coarse vector with +inf in one value per test position: the first aggregate, one in the middle, the lone last one."""
    nc = (n + 1) // 2
    return [0, (nc ** dim) // 2, nc ** dim - 1]


@pytest.mark.parametrize("n", ODD_2D)
def test_mg_stage_transfers(Blab, O, n):
    rp, ci, cases = transfer_cases(n, 2)
    nc = (n + 1) // 2
    d_rp, d_ci = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci)
    try:
        for label, va, z, r, want in cases:
            d_va, dz, dr, dc = GuardedBytes(Blab, va), Guarded(Blab, z), Guarded(Blab, r), Guarded(Blab, np.full(nc * nc, np.nan))
            try:
                a = Blab.MgStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
                assert Blab.mg_stage("residual_restrict", a) == 0
                assert same_bits_nan_as_class(dc.read(), want), (n, label)
                assert same_bits(dz.read(), z) and same_bits(dr.read(), r) and same_bits(d_va.read(), va), (n, label)
            finally:
                for g in (d_va, dz, dr, dc):
                    g.free()
        z = clean_columns(n)[3]
        for at in coarse_poison(n, 2):
            ec = clean_columns(n)[4][:nc * nc].copy()
            ec[at] = np.inf
            want = O.axpy(2.0, MG.prolong(ec, n), z)
            assert 1 <= np.isinf(want).sum() <= 4
            dz, de = Guarded(Blab, z), Guarded(Blab, ec)
            try:
                assert Blab.mg_stage("prolong", Blab.MgStageArgs(n=n, z=dz.ptr, coarse=de.ptr)) == 0
                assert same_bits_nan_as_class(dz.read(), want), (n, at)
                assert same_bits(de.read(), ec)
            finally:
                dz.free(), de.free()
    finally:
        d_rp.free(), d_ci.free()


def multi_transfers(Blab, O, stage_call, names, n, dim, k):
    """The batched residual + restriction and prolongation + correction with the poison in column k // 2 of the block only."""
    R = MG if dim == 2 else M3
    rp, ci, cases = transfer_cases(n, dim)
    nc = (n + 1) // 2
    clean = clean_columns(n, dim)
    jp = k // 2
    d_rp, d_ci = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci)
    try:
        for label, va, z, r, want in cases:
            Z, Rk = clean[:k].copy(), clean[::-1][:k].copy()
            Z[jp], Rk[jp] = z, r
            zb, rb = interleaved(Z, k), interleaved(Rk, k)
            d_va, dz, dr = GuardedBytes(Blab, va), Guarded(Blab, zb), Guarded(Blab, rb)
            dc = Guarded(Blab, np.full(nc ** dim * k, np.nan))
            try:
                a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
                assert stage_call(names[0], k, a) == 0
                got = dc.read()
                for j in range(k):
                    wj = want if j == jp else clean_coarse_residual(n, dim, label == "coefficient", j)
                    assert same_bits_nan_as_class(column(got, k, j), wj), (n, k, label, j)
                    if label != "coefficient" and j != jp:
                        assert np.isfinite(wj).all()
                assert same_bits(dz.read(), zb) and same_bits(dr.read(), rb) and same_bits(d_va.read(), va), (n, k, label)
            finally:
                for g in (d_va, dz, dr, dc):
                    g.free()
        Z = clean[:k].copy()
        zb = interleaved(Z, k)
        for at in coarse_poison(n, dim):
            E = clean[::-1][:k, :nc ** dim].copy()
            E[jp, at] = np.inf
            eb = interleaved(E, k)
            dz, de = Guarded(Blab, zb), Guarded(Blab, eb)
            try:
                assert stage_call(names[1], k, Blab.MgMultiStageArgs(n=n, z=dz.ptr, coarse=de.ptr)) == 0
                got = dz.read()
                for j in range(k):
                    wj = O.axpy(2.0, R.prolong(E[j], n), Z[j])
                    members = int(np.isinf(wj).sum())  # its 4 (8) members, fewer at the odd edge; no other column sees it
                    assert (1 <= members <= 2 ** dim) if j == jp else members == 0, (n, k, at, j, members)
                    assert same_bits_nan_as_class(column(got, k, j), wj), (n, k, at, j)
                assert same_bits(de.read(), eb)
            finally:
                dz.free(), de.free()
    finally:
        d_rp.free(), d_ci.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ODD_2D)
def test_mg_multi_stage_transfers(Blab, O, n, k):
    multi_transfers(Blab, O, Blab.mg_multi_stage, ("residual_restrict", "prolong"), n, 2, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ODD_3D)
def test_mg_multi_stage3d_transfers(Blab, O, n, k):
    multi_transfers(Blab, O, Blab.mg_multi_stage3d, ("residual_restrict3d", "prolong3d"), n, 3, k)


@pytest.mark.parametrize("planter", P.PLANTERS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", P.GRIDS_3D)
def test_the_3d_block_product_in_both_kinds(Blab, O, n, k, planter):
    """stencil7_spmm and spmm/csr on a poisoned 3-D system, the poison in column k // 2: every column the oracle's CSR product, and the
    two kinds equal to each other, both under the NaN-class rule."""
    s = P.system(n, planter, 3)
    X = block_of(s, k)
    xb = interleaved(X, k)
    d_rp, d_ci, d_va, dz = GuardedBytes(Blab, s.rp), GuardedBytes(Blab, s.ci), GuardedBytes(Blab, s.va), Guarded(Blab, xb)
    got = {}
    try:
        for stage in ("stencil7_spmm", "spmm_csr"):
            dy = Guarded(Blab, np.full(n ** 3 * k, np.nan))
            try:
                a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, d=dy.ptr)
                assert Blab.mg_multi_stage3d(stage, k, a) == 0
                got[stage] = dy.read()
            finally:
                dy.free()
        for j in range(k):
            wj = O.spmv_csr(s.rp, s.ci, s.va, X[j])
            for stage in got:
                assert same_bits_nan_as_class(column(got[stage], k, j), wj), (stage, n, k, planter, j)
            if planter != "coef_inf" and j != k // 2:
                assert np.isfinite(wj).all()
        assert same_bits_nan_as_class(got["stencil7_spmm"], got["spmm_csr"])
        assert same_bits_nan_as_class(got["spmm_csr"], got["stencil7_spmm"])
        assert same_bits(dz.read(), xb) and same_bits(d_va.read(), s.va)
    finally:
        for g in (d_rp, d_ci, d_va, dz):
            g.free()


# ---------------------------------------------------------------- the single-rank CG slab
BETA = 0.37
RR_OLD, PAP = 1.7, 3.1  # alpha = rr_old / pAp on the device


def partials_where_finite(got, want, n, what):
    """A dot partial is compared where the oracle's own partial is finite (elsewhere the order of a tree decides between inf and NaN).
    From n = 129 on most partials must be finite; on the 9 x 9 grid nearly every grid row holds a poisoned value, there the
    comparison covers whatever is finite, possibly nothing."""
    assert len(got) == len(want), what
    live = np.isfinite(want)
    assert n == 9 or 2 * live.sum() > len(want), (what, n, int(live.sum()), len(want))
    differ = np.flatnonzero(live & bits_differ(got, want))
    assert len(differ) == 0, (what, differ[:8])


def bits_differ(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) != np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


def slab_stages(slab, O, rp, ci, va, n, x, clean, planes, first_stage):
    """Every stage of the loop that takes host vectors, each against the oracle's product of what the stage multiplies and the
    restated partials (reduction_restatement):
    - spmv in its in-loop form with its p.Ap partials, and as a plain product;
    - planes only (the CSR form has no such launch): the direction update inside the block SpMV, the poison in r and then in p;
    - first_stage: iteration 0's launch on b = x. Only where a solve would take b as p0: the planes form of a matrix whose rows
      sum to +0.0 over zero operands (slab_decisions.hpp b_is_p0), which a matrix with an inf coefficient is not (inf * 0).
    The r update that recomputes A p (update_r_from_stage) needs more of the slab: see recomputing_r_update."""
    product = lambda v: O.spmv_stencil5(rp, ci, va, v, n)
    with np.errstate(invalid="ignore"):
        slab.set_option("spmv_with_dot", 1)
        want = product(x)
        assert same_bits_nan_as_class(slab.spmv(x), want)
        partials, _ = slab.spmv_dot()
        partials_where_finite(partials, RR.rowlds_partials(x, want, n), n, "spmv_dot")
        slab.set_option("spmv_with_dot", 0)
        assert same_bits_nan_as_class(slab.spmv(x), want)
        for r, p in ((x, clean), (clean, x)) if planes else ():
            want_p = r + BETA * p
            want_Ap = product(want_p)
            p_out, Ap, partials, _ = slab.direction_spmv(r, p, BETA)
            assert same_bits_nan_as_class(p_out, want_p) and same_bits_nan_as_class(Ap, want_Ap)
            partials_where_finite(partials, RR.rowlds_partials(want_p, want_Ap, n), n, "direction_spmv")
        if first_stage:
            slab.set_vectors(b=x)
            assert slab.first_form() == 1
            for reverse in (True, False):
                Ab, pAp_partials, bb_partials, _, _ = slab.first_stage(reverse=reverse)
                assert same_bits_nan_as_class(Ab, want)
                partials_where_finite(pAp_partials, RR.rowlds_partials(x, want, n), n, "first_stage p.Ap")
                partials_where_finite(bb_partials, RR.rowlds_partials(x, x, n), n, "first_stage b.b")
            assert same_bits(slab.stored_b(), x)
        elif planes:
            assert slab.first_form() == 0  # an inf coefficient: A 0 is not +0.0, b cannot stand for r0


def recomputing_r_update(slab, O, rp, ci, va, n, R, x, want_fast):
    """Iteration 0's r update from the one vector that is r0 and p0 (update_r_from_stage, recompute=True): A x is recomputed on the
    fast row blocks -- the A p handed in holds NaN there, so the launch must not read it -- and read on the slow ones. The launch
    decides per row block, so every row block must be all-fast or all-slow (skew_geometry.hpp skew_eligible; CgSlab.ap_form()):
    a matrix without a uniform tile is all-slow (want_fast False: everything is read), the anisotropic one is fast but for the
    blocks of the grid's first and last grid row. r = fma(-alpha, A x, x) and its r.r partials against the oracle's."""
    assert slab.ap_form()[2]
    m = np.asarray(slab.block_map(0)).reshape(-1, T.col_tiles(n))
    fast = np.repeat(np.repeat((m == 1).all(axis=1), R)[:n], n)
    assert (fast.any() and not fast.all()) if want_fast else not fast.any()
    with np.errstate(invalid="ignore"):
        Ax = O.spmv_stencil5(rp, ci, va, x, n)
        want_r = O.axpy(-(RR_OLD / PAP), Ax, x)
        for reverse in (False, True):
            half = np.where(fast, np.nan, Ax)
            r_out, src_back, partials = slab.update_r_from_stage(x, half, RR_OLD, PAP, recompute=True, reverse=reverse)
            assert same_bits_nan_as_class(r_out, want_r) and same_bits(src_back, x)
            partials_where_finite(partials, RR.residual_partials(want_r), n, "update_r_from")


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("planter", ["x_inf", "coef_inf"])
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_cg_slab_on_a_symmetric_random_matrix(Blab, O, monkeypatch, n, planter, R):
    """No uniform tile: every block tile loads its coefficients, from the planes and (LAB option csr_coefficients) from the CSR."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "2")
    Blab.lib().spmv_amd_reset_host_matrices()
    s = P.slab_system(n, planter)
    slab = Blab.CgSlab.from_matrix(host_matrix(Blab, s))
    try:
        assert slab.variant() == "stencil5/row-lds" and slab.coefficient_form() == 1 and slab.uniform_tiles()[0] == 0
        slab.set_block_rows(R)
        slab.set_option("fused_direction", 2)
        clean = clean_columns(n)[5]
        for csr in (0, 1):
            slab.set_option("csr_coefficients", csr)
            assert slab.coefficient_form() == 1 - csr
            slab_stages(slab, O, s.rp, s.ci, s.va, n, s.x, clean, planes=csr == 0, first_stage=(csr == 0 and planter == "x_inf"))
            if csr == 0:
                recomputing_r_update(slab, O, s.rp, s.ci, s.va, n, R, s.x, want_fast=False)
            else:  # the launches that read the planes do not exist in the CSR form
                with pytest.raises(RuntimeError):
                    slab.direction_spmv(clean, clean, BETA)
                with pytest.raises(RuntimeError):
                    slab.update_r_from_stage(clean, clean, RR_OLD, PAP, recompute=True)
    finally:
        slab.destroy()
        Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name,planter", P.UNIFORM_TABLE)
def test_cg_slab_on_uniform_tiles(Blab, O, monkeypatch, name, planter, R):
    """The uniform-tile path multiplies by the slab-wide quintuple. A poisoned coefficient makes its tile class 0 (and only its tile), a
    poisoned x changes no class; the r update that recomputes A p on the fast row blocks reads no A p there."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "8")
    Blab.lib().spmv_amd_reset_host_matrices()
    s = P.uniform_system(name, planter)
    n, x = s.n, s.x
    ct = T.col_tiles(n)
    slab = Blab.CgSlab.from_matrix(host_matrix(Blab, s))
    try:
        assert slab.variant() == "stencil5/row-lds" and slab.coefficient_form() == 1
        cls = slab.tile_classes().reshape(n, ct)
        want_cls = np.zeros((n, ct), dtype=np.uint8)
        want_cls[1:n - 1] = 1
        if planter == "coef_inf":
            want_cls[s.seams["tile"]] = 0
        assert np.array_equal(cls, want_cls) and slab.uniform_tiles() == (int(want_cls.sum()), (n - 2) * ct)
        slab.set_block_rows(R)
        slab.set_option("fused_direction", 2)
        slab_stages(slab, O, s.rp, s.ci, s.va, n, x, clean_columns(n)[5], planes=True, first_stage=planter == "x_inf")
        assert slab.coefficient_form() == 1
        if planter == "x_inf":
            recomputing_r_update(slab, O, s.rp, s.ci, s.va, n, R, x, want_fast=True)
        else:  # the poisoned tile's row block is neither all-fast nor all-slow: the slab does not take the recomputing form
            assert not slab.ap_form()[2]
            with pytest.raises(RuntimeError):
                slab.update_r_from_stage(x, x, RR_OLD, PAP, recompute=True)
    finally:
        slab.destroy()
        Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- slabs with halos
@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("matrix", ["generator", "random"])
def test_two_slabs_with_poisoned_halo_rows(Blab, O, monkeypatch, matrix, rank):
    """P = 2 over the staged transport at n = 130 (65 grid rows each, a last tile of two columns): +inf at the seam columns of the
    grid row in front of the slab and of the one behind it (the neighbour's rows, which reach the slab as halos only). Only the slab's
    first grid row, respectively its last, may see it -- on uniform tiles (the generator's matrix) and on streamed coefficients, in
    the one-row kernel and on block tiles, in the plain and the in-loop form."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "2")
    Blab.lib().spmv_amd_reset_host_matrices()
    n, world = 130, 2
    if matrix == "generator":
        e = O.stencil5_coo(n)
        rp, ci, va = O.build_csr(e, n * n)
    else:
        s = P.slab_system(n, "x_inf")
        rp, ci, va, e = s.rp, s.ci, s.va, P.entries_of(s.rp, s.ci, s.va)
    comm = Blab.Comm.staged(rank, world, lambda *a: 0, lambda *a: 0)
    slab = Blab.CgSlab.from_matrix(Blab.HostMatrix(e, n * n, n * n, n), comm)
    try:
        off, nl = slab.row_offset, slab.n_local
        assert (off, nl) == O.partition_rows(n * n, world, rank) and off % n == 0 and nl % n == 0
        assert slab.variant() == "stencil5/row-lds" and slab.coefficient_form() == 1
        x = clean_columns(n)[7].copy()
        front, behind = off // n - 1, (off + nl) // n
        for gi in (front, behind):
            if 0 <= gi < n:
                x[gi * n + np.array(P.seam_columns(n))] = np.inf
        base = rp[off]
        lrp = (rp[off:off + nl + 1] - base).astype(np.int32)
        hp = x[off - n:off] if rank > 0 else None
        hn = x[off + nl:off + nl + n] if rank < world - 1 else None
        assert np.isfinite(x[off:off + nl]).all() and (np.isinf(hp).sum() if rank else np.isinf(hn).sum()) == len(P.seam_columns(n))
        want = O.spmv_halo(lrp, ci[base:], va[base:], x[off:off + nl], hp, hn, off, n * n, n)
        seen = np.flatnonzero(~np.isfinite(want))
        edge_row = 0 if rank else nl // n - 1
        assert np.array_equal(seen, edge_row * n + np.array(P.seam_columns(n)))
        for R in (0, 4, 8):
            slab.set_block_rows(R)
            for with_dot in (1, 0):
                slab.set_option("spmv_with_dot", with_dot)
                assert same_bits_nan_as_class(slab.spmv(x), want), (matrix, rank, R, with_dot)
    finally:
        slab.destroy()
        comm.destroy()
        Blab.lib().spmv_amd_reset_host_matrices()
