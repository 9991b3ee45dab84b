"""numpy restatement of the CG slab's tile classifier (csrc/spmv_kernels.hip classify_tiles_kernel, csrc/cg_slab_create.hip classify_tiles;
kernels.hpp SymPlanes). Test infrastructure only.

A row-lds tile is TILE = 128 columns of one grid row. A tile of a global grid row 1 .. n-2 is uniform (class 1) if every coefficient
its fma chains multiply equals, as a 64-bit pattern, the matching member of one slab-wide quintuple (W, C, E, N, S): interior columns
W, C, E, N, S; column 0 N, C, E, S; column n-1 N, W, C, S; columns past n do not exist. The grid's first and last grid row walk the
CSR in every form: class 0, not counted. The quintuple is the CSR row of the grid point (middle plane-evaluated grid row of the
slab, column n // 2)."""
import numpy as np

TILE = 128


def col_tiles(n):
    return (n + TILE - 1) // TILE


def plane_rows(n, row_offset, n_local):
    """Global grid rows [lo, hi) of the slab that are evaluated from the planes."""
    gfirst, rows = row_offset // n, n_local // n
    return max(gfirst, 1), min(gfirst + rows, n - 1)


def quintuple(rp, va, n, row_offset, n_local):
    """(W, C, E, N, S) of the slab, or None for a slab without a plane-evaluated grid row (or a grid of fewer than three columns)."""
    lo, hi = plane_rows(n, row_offset, n_local)
    if hi <= lo or n < 3:
        return None
    g = (lo + (hi - lo) // 2) * n + n // 2
    row = np.asarray(va[rp[g]:rp[g + 1]], dtype=np.float64)  # [N, W, C, E, S]
    assert len(row) == 5
    return np.array([row[1], row[2], row[3], row[0], row[4]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def classify(rp, ci, va, n, row_offset, n_local, q=None):
    """Class map (uint8 [local grid rows, col_tiles(n)]), uniform count, total -- of the slab of global rows [row_offset,
    row_offset + n_local) (whole grid rows) of the n x n 5-point CSR (rp, ci, va; global). (None, 0, 0) where the library keeps no map."""
    assert row_offset % n == 0 and n_local % n == 0
    rp = np.asarray(rp, dtype=np.int64)
    va = np.asarray(va, dtype=np.float64)
    if q is None:
        q = quintuple(rp, va, n, row_offset, n_local)
    if q is None:
        return None, 0, 0
    qw, qc, qe, qn, qs = (_bits(np.array([v]))[0] for v in q)
    gfirst, rows = row_offset // n, n_local // n
    lo, hi = plane_rows(n, row_offset, n_local)
    ct = col_tiles(n)
    cls = np.zeros((rows, ct), dtype=np.uint8)
    j = np.arange(n)
    for gi in range(lo, hi):
        g = gi * n + j
        first, last = rp[g], rp[g + 1] - 1
        kc = np.where(j > 0, 2, 1)
        ok = (_bits(va[first]) == qn) & (_bits(va[first + kc]) == qc) & (_bits(va[last]) == qs)
        ok[1:] &= _bits(va[first[1:] + 1]) == qw          # column 0 has no W
        ok[:-1] &= _bits(va[first[:-1] + kc[:-1] + 1]) == qe  # column n-1 has no E
        pad = np.ones(ct * TILE, dtype=bool)
        pad[:n] = ok
        cls[gi - gfirst] = pad.reshape(ct, TILE).all(axis=1)
    return cls, int(cls.sum()), (hi - lo) * ct


# ---- hand-built matrices for the tests (generator's stencil: centre 5, off-diagonals -1) ----

def set_entry(e, row, col, value):
    k = np.flatnonzero((e["row"] == row) & (e["col"] == col))
    assert len(k) == 1, (row, col)
    e["value"][k[0]] = value


def set_edge(e, a, b, value):
    """Both directions of one undirected edge: the matrix stays bitwise symmetric, so a slab keeps its planes."""
    set_entry(e, a, b, value)
    set_entry(e, b, a, value)


MIXED_N = 640  # five tiles per grid row; P = 2 cuts between grid rows 319 and 320


def mixed_perturbations(n=MIXED_N):
    """(centres, edges) as lists of grid positions: centres [(gi, j)], edges [((gi, j), (gi', j'))]. The awkward places: columns 0,
    1, 127, 128 and n-1; grid rows 1 and n-2; the last local grid row of the first P = 2 slab and the first of the second; a vertical
    edge (flips the tile in both grid rows), one across the P = 2 cut, and a horizontal edge across a tile boundary (flips both
    tiles) -- in both halves of the grid, so that every slab of P = 1 and P = 2 holds at least 8 tiles of each class."""
    half = n // 2
    centres = [(1, 300), (n - 2, 300), (half - 1, 200), (half, 200)]
    edges = [((half - 1, 500), (half, 500))]
    for base in (0, half + 80):
        centres += [(base + 5, 0), (base + 10, 1), (base + 15, 127), (base + 20, 128), (base + 25, n - 1)]
        edges += [((base + 100, 50), (base + 101, 50)), ((base + 200, 127), (base + 200, 128))]
    return centres, edges


def mixed_coo(O, n=MIXED_N):
    """The generator's matrix with mixed_perturbations applied (still symmetric, still diagonally dominant: SPD)."""
    e = O.stencil5_coo(n)
    centres, edges = mixed_perturbations(n)
    for gi, j in centres:
        set_entry(e, gi * n + j, gi * n + j, 5.5)
    for (ga, ja), (gb, jb) in edges:
        set_edge(e, ga * n + ja, gb * n + jb, -1.25)
    return e


def mixed_expected_class0(n=MIXED_N):
    """The (grid row, tile) pairs mixed_perturbations must flip, derived by hand from the list (not by the classifier)."""
    centres, edges = mixed_perturbations(n)
    out = {(gi, j // TILE) for gi, j in centres}
    for (ga, ja), (gb, jb) in edges:
        out |= {(ga, ja // TILE), (gb, jb // TILE)}
    return out
