"""The poisoned systems of tests/poison.py on the CPU alone: the oracle's non-finite rows are exactly the rows whose CSR row holds a
poisoned column or coefficient, that set is non-empty and small and covers every seam position, the 2-D signed-zero contract of
csrc/stencil_row_device.hpp holds in the oracle, and the NaN-class comparator accepts and rejects what it should. With these a failure
of tests/test_poison_gpu.py can only be the kernel's."""
import numpy as np
import pytest
import scipy.sparse as sp

import chebyshev_restatement as CR
import multigrid3d_restatement as M3
import multigrid_restatement as MG
import poison as P
from bitwise import same_bits, same_bits_nan_as_class


def oracle_products(O, s):
    if s.dim == 2:
        return [O.spmv_stencil5(s.rp, s.ci, s.va, s.x, s.n), O.spmv_csr(s.rp, s.ci, s.va, s.x)]
    return [O.spmv_csr(s.rp, s.ci, s.va, s.x)]


@pytest.mark.parametrize("n,planter,dim,clamp_targets", [c for c in P.TABLE if c[1] != "x_negzero"])
def test_the_poisoned_footprint_is_the_matrix_adjacency(O, n, planter, dim, clamp_targets):
    s = P.system(n, planter, dim, clamp_targets)
    rows = n ** dim
    want = P.poisoned_rows(s.rp, s.ci, s.x_at, s.coef_at)
    assert len(want) > 0
    if n >= 65:
        assert len(want) < 0.01 * rows, (len(want), rows)
    for y in oracle_products(O, s):
        assert np.array_equal(np.flatnonzero(~np.isfinite(y)), want)
    # every seam position, read back from the poisoned data itself
    if planter in ("x_inf", "x_inf_pairs"):
        at = np.flatnonzero(np.isinf(s.x))
        assert np.array_equal(at, s.x_at) and np.isfinite(s.va).all()
        cols = P.seam_columns(n) if planter == "x_inf" else P.pair_columns(n)
        assert set(P.seam_columns(n)) <= set(cols) and (planter == "x_inf" or n < 127 or 126 in cols)
        assert sorted(set(at % n)) == cols == s.seams["columns"]
        assert sorted(set((at // n) % n)) == P.edge_rows(n) == s.seams["rows"]
        if dim == 3:
            assert sorted(set(at // (n * n))) == P.edge_rows(n) == s.seams["planes"]
        assert set(P.lone_last(n)) <= set(at % n) and set(P.lone_last(n)) <= set((at // n) % n)
    else:
        at = np.flatnonzero(np.isinf(s.va))
        assert np.array_equal(at, s.coef_at) and np.isfinite(s.x).all()
        ends = {0, len(s.ci) - 1}
        assert ends <= set(at) if clamp_targets else not (ends & set(at))
        row, col = P.row_of_entry(s.rp)[at], s.ci[at]
        horizontal = np.abs(row - col) == 1
        assert sorted(set(row[horizontal] % n)) == P.seam_columns(n)  # a W or E entry at every seam column
        grid_row_starts = s.rp[np.arange(n, rows, n)]  # (but the matrix's own first entry)
        first, in_front = at[np.isin(at, grid_row_starts)], at[np.isin(at + 1, grid_row_starts)]
        assert len(first) > 0 and len(in_front) > 0  # a grid row's first entry, and the entry in front of a grid row's first
        assert not set(row[np.isin(at, first)]) & set(row[np.isin(at, in_front)] + 1)  # in different rows: each shows alone


@pytest.mark.parametrize("n,planter", P.SLAB_TABLE)
def test_the_slab_systems(O, n, planter):
    """The same for the CG slab's systems, which are bitwise symmetric with a positive diagonal (also under the poison)."""
    s = P.slab_system(n, planter)
    want = P.poisoned_rows(s.rp, s.ci, s.x_at, s.coef_at)
    assert 0 < len(want) and (n < 65 or len(want) < 0.01 * n * n)
    for y in oracle_products(O, s):
        assert np.array_equal(np.flatnonzero(~np.isfinite(y)), want)
    A = sp.csr_matrix((s.va, s.ci, s.rp), shape=(n * n, n * n))
    T = sp.csr_matrix(A.T)
    T.sort_indices()
    assert np.array_equal(T.indices, s.ci) and same_bits(T.data, s.va) and (A.diagonal() > 0.0).all()
    if planter == "x_inf":
        at = np.flatnonzero(np.isinf(s.x))
        assert sorted(set(at % n)) == P.seam_columns(n) and sorted(set(at // n)) == P.slab_rows(n)
        for block in (4, 8):
            seams = list(range(block, n, block))
            assert {r for q in (seams[0], seams[-1]) for r in (q - 1, q)} <= set(at // n)
        assert set(at // n) <= set(P.seam_rows(n, 4)) | set(P.seam_rows(n, 8))
    else:
        at = np.flatnonzero(np.isinf(s.va))
        row, col = P.row_of_entry(s.rp)[at], s.ci[at]
        # (the other direction of a seam column's W or E entry sits in the neighbouring column)
        assert {0, len(s.ci) - 1} <= set(at) and set(P.seam_columns(n)) <= set(row[np.abs(row - col) == 1] % n)


@pytest.mark.parametrize("name,planter", P.UNIFORM_TABLE)
def test_the_uniform_tile_systems(O, name, planter):
    s = P.uniform_system(name, planter)
    n = s.n
    want = P.poisoned_rows(s.rp, s.ci, s.x_at, s.coef_at)
    assert 0 < len(want) < 0.01 * n * n
    for y in oracle_products(O, s):
        assert np.array_equal(np.flatnonzero(~np.isfinite(y)), want)
    if planter == "x_inf":
        at = np.flatnonzero(np.isinf(s.x))
        assert sorted(set(at % n)) == P.seam_columns(n) and sorted(set(at // n)) == P.slab_rows(n) and np.isfinite(s.va).all()
    else:
        gi, tile = s.seams["tile"]
        assert np.isfinite(s.x).all() and 1 <= gi < n - 1
        assert np.array_equal(want, [gi * n + 63, gi * n + 64]) and {63 // P.TILE, 64 // P.TILE} == {tile}  # both ends in one tile


def test_the_padding_case(O):
    """Nothing holds the poisoned columns: the footprint is empty and the oracle's product finite."""
    e, rows, cols, x = P.padding_case()
    rp, ci, va = O.build_csr(e, rows)
    at = np.flatnonzero(np.isinf(x))
    assert np.array_equal(at, [0, cols - 1]) and len(P.poisoned_rows(rp, ci, at, [])) == 0
    assert np.isfinite(O.spmv_csr(rp, ci, va, x)).all() and (np.diff(rp) == 0).any() and np.diff(rp).max() > np.diff(rp).min() + 3


@pytest.mark.parametrize("case", P.CHEBYSHEV_CASES)
@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_the_chebyshev_systems(O, n, case):
    """One fused step spreads the poison over the matrix's adjacency of it, a second over the adjacency of that; creation's checks
    on the diagonal (finite, non-zero, one sign) hold, and dinv is +inf exactly where the "dinv" case wants it."""
    s = P.chebyshev_system(n, case)
    diagonal = s.va[P.row_of_entry(s.rp) == s.ci]
    assert np.isfinite(diagonal).all() and (diagonal > 0.0).all()
    with np.errstate(over="ignore"):
        dinv = 1.0 / diagonal
    assert np.array_equal(np.flatnonzero(np.isinf(dinv)), s.x_at if case == "dinv" else [])
    assert np.array_equal(np.flatnonzero(np.isinf(s.x)), s.x_at if case == "r" else [])
    if case != "coefficient":
        at = s.x_at
        assert sorted(set(at % n)) == P.seam_columns(n) and sorted(set(at // n)) == P.edge_rows(n)
    ring1 = P.poisoned_rows(s.rp, s.ci, s.x_at, s.coef_at)
    ring2 = P.poisoned_rows(s.rp, s.ci, ring1, [])
    assert 0 < len(ring1) < len(ring2) and (n < 65 or len(ring2) < 0.01 * n * n)
    matvec = lambda v: O.spmv_stencil5(s.rp, s.ci, s.va, v, n)
    with np.errstate(invalid="ignore", over="ignore"):
        for degree, want in ((1, ring1), (2, ring2)):
            z = CR.make_apply(matvec, dinv, list(CR.coefficients(degree, *P.CHEBYSHEV_BOUNDS)), fma=O.axpy)(s.x)
            assert np.array_equal(np.flatnonzero(~np.isfinite(z)), want), (degree, len(want))


@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_seam_lists(n):
    cols = P.seam_columns(n)
    assert cols == sorted(set(cols)) and cols[0] == 0 and cols[-1] == n - 1 and all(0 <= c < n for c in cols)
    assert {c for c in (0, 1, 63, 64, 65, 127, 128, 129, n - 2, n - 1) if c < n} <= set(cols)
    if n == 257:
        assert cols == [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
    for block in (4, 8):
        rows = P.seam_rows(n, block)
        assert {0, 1, n - 2, n - 1} <= set(rows) and all(0 <= r < n for r in rows)
        assert {r for s in range(block, n, block) for r in (s - 1, s)} <= set(rows)
        assert len(rows) == len(set(rows)) <= 4 + 2 * ((n - 1) // block)
    assert P.lone_last(n) == ([n - 1] if n % 2 else [])
    assert len(P.positions_3d(n)) == len(P.positions_2d(n)) == max(len(cols), len(P.edge_rows(n)))


@pytest.mark.parametrize("n", P.GRIDS_2D)
def test_signed_zeros_of_the_2d_family(O, n):
    """An interior row starts with the bare product vW xW and so returns -0.0 when every product is -0.0; an edge-column row starts
    fma(v, x, +0.0) and cannot; the CSR loop starts every row at +0.0 (csrc/stencil_row_device.hpp)."""
    s = P.system(n, "x_negzero")
    i = s.seams["rows"][1]
    assert (s.va > 0.0).all() and np.signbit(s.x[(i - 1) * n:(i + 2) * n]).all() and (s.x[(i - 1) * n:(i + 2) * n] == 0.0).all()
    st = O.spmv_stencil5(s.rp, s.ci, s.va, s.x, n)[i * n:(i + 1) * n]
    assert (st == 0.0).all()
    assert np.signbit(st[1:n - 1]).all(), "interior columns: -0.0"
    assert not np.signbit(st[0]) and not np.signbit(st[n - 1]), "columns 0 and n-1: +0.0"
    loop = O.spmv_csr(s.rp, s.ci, s.va, s.x)[i * n:(i + 1) * n]
    assert (loop == 0.0).all() and not np.signbit(loop).any()
    assert np.isfinite(O.spmv_stencil5(s.rp, s.ci, s.va, s.x, n)).all()


@pytest.mark.parametrize("n", P.GRIDS_3D)
def test_signed_zeros_of_the_3d_family(O, n):
    s = P.system(n, "x_negzero", 3)
    k = s.seams["planes"][1]
    y = O.spmv_csr(s.rp, s.ci, s.va, s.x)
    plane = y[k * n * n:(k + 1) * n * n]
    assert np.isfinite(y).all() and (plane == 0.0).all() and not np.signbit(plane).any()


@pytest.mark.parametrize("n", [9, 129])
def test_transfers_spread_a_poison_over_its_aggregate_only(n):
    """restrict: the aggregates whose members hold +inf, no other; prolong: one coarse value reaches its 4 (8) members, fewer at the
    odd edge."""
    nc = (n + 1) // 2
    for dim, R in ((2, MG), (3, M3)):
        if dim == 3 and n > 9:
            continue
        t = np.ones(n ** dim)
        at = P.flat(P.positions_2d(n) if dim == 2 else P.positions_3d(n), n)
        t[at] = np.inf
        coarse = np.zeros(nc ** dim, dtype=bool)
        idx = at.copy()
        c, scale = np.zeros(len(at), dtype=np.int64), 1
        for _ in range(dim):
            c += (idx % n) // 2 * scale
            idx, scale = idx // n, scale * nc
        coarse[c] = True
        assert np.array_equal(~np.isfinite(R.restrict(t, n)), coarse)
        for corner in (0, nc ** dim - 1):
            ec = np.ones(nc ** dim)
            ec[corner] = np.inf
            members = int(np.isinf(R.prolong(ec, n)).sum())
            assert members == (2 ** dim if corner == 0 or n % 2 == 0 else 1), (dim, corner, members)


def test_the_nan_class_comparator():
    pnan = np.array([np.nan])
    nnan = np.copysign(pnan, -1.0)
    payload = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)
    assert np.signbit(nnan[0]) and not np.signbit(pnan[0])
    want = np.array([1.5, -0.0, 0.0, np.inf, -np.inf, np.nan, 2.0])
    assert same_bits_nan_as_class(want, want)
    for nan in (pnan, nnan, payload):  # a NaN of either sign, of any payload, where NaN is wanted
        got = want.copy()
        got[5] = nan[0]
        assert same_bits_nan_as_class(got, want)
        assert same_bits_nan_as_class(got.reshape(1, -1), want.reshape(1, -1))
    for at in (0, 1, 2, 3, 4):  # NaN where a finite value, a zero or an inf is wanted
        got = want.copy()
        got[at] = np.nan
        with pytest.raises(AssertionError, match="differ"):
            same_bits_nan_as_class(got, want)
    for at, value in ((1, 0.0), (2, -0.0), (3, -np.inf), (4, np.inf), (5, np.inf), (5, 0.0), (0, np.nextafter(1.5, 2.0)), (3, 1.0)):
        got = want.copy()
        got[at] = value
        assert not same_bits(got, want)
        with pytest.raises(AssertionError, match="differ"):
            same_bits_nan_as_class(got, want)
    with pytest.raises(AssertionError, match=r"1 non-finite where a finite value is wanted \(first at \[6\]\), 1 finite where a non-finite"):
        got = want.copy()
        got[6], got[3] = np.inf, 7.0
        same_bits_nan_as_class(got, want)
    with pytest.raises(AssertionError):
        same_bits_nan_as_class(want[:3], want)
