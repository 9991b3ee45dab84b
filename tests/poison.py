"""Poisoned inputs for the stencil kernels (tests/test_poison_host.py, tests/test_poison_gpu.py). Test infrastructure only.

A kernel that reads a value its row does not hold and cancels it -- multiplies it by 0.0, adds it to a sum -- changes no bit on finite
data. With +inf at such a place the product is NaN, with -0.0 over a whole neighbourhood a sum started at +0.0 differs from a bare
product in its sign. This module says WHERE a 128-column tile of two 64-lane halves, a block of grid rows and the multigrid pair walk
can read such a value (the seam positions), plants the poison there, and states which rows may see it: those whose CSR row holds a
poisoned column or a poisoned coefficient, by plain indexing of row_ptr / col_idx. Grid point (i, j) of an n x n grid is row i n + j,
point (k, i, j) of an n^3 grid is row k n^2 + i n + j; every matrix is a sorted CSR (columns ascending: [N, W, C, E, S] in 2-D,
[D, N, W, C, E, S, U] in 3-D, absent neighbours left out)."""
import collections
import functools

import numpy as np

from matrices import ENTRY_DTYPE

TILE = 128
# one short tile; a second tile of one live column; of two; a middle tile with both outer neighbours in memory
GRIDS_2D = (9, 129, 130, 257)
GRIDS_3D = (6, 65, 129)        # row-direct only; one live column in the tile's second half; a second tile of one live column
PLANTERS = ("x_inf", "x_negzero", "coef_inf")


# ---------------------------------------------------------------- seam positions
def seam_columns(n, tile=TILE):
    """The columns where a tile of two halves can go wrong: 0, 1, the last lane of the first half and the first two of the second, the
    tile's last column and the first two of the next tile -- around every tile start --, and the grid row's last two columns."""
    half = tile // 2
    at = {n - 2, n - 1}
    for t in range(0, n, tile):
        at |= {t, t + 1, t + half - 1, t + half, t + half + 1, t + tile - 1, t + tile, t + tile + 1}
    return sorted(c for c in at if 0 <= c < n)


def pair_columns(n, tile=TILE):
    """seam_columns for the multigrid pair walk, where lane l holds columns 2 l and 2 l + 1 of the tile: the first column of the last
    lane's pair as well (its E side comes from the next lane, or from memory in lane 63), as column 1 is the second of lane 0's."""
    return sorted(set(seam_columns(n, tile)) | {t + tile - 2 for t in range(0, n, tile) if t + tile - 2 < n})


def seam_rows(n, block):
    """Grid rows 0, 1, n-2, n-1 and the rows on either side of every seam between blocks of `block` grid rows (4 or 8:
    set_block_rows). The full list: the slab's cases plant at slab_rows, a subset of it that keeps the footprint under 1 % of a
    129 grid, and tests/test_poison_host.py holds that subset against this list."""
    at = {0, 1, n - 2, n - 1}
    for s in range(block, n, block):
        at |= {s - 1, s}
    return sorted(r for r in at if 0 <= r < n)


def lone_last(n):
    """The multigrid pair walk's lone last row / column / plane: index n-1 of an odd n (an aggregate of fewer members), else nothing."""
    return [n - 1] if n % 2 == 1 else []


def slab_rows(n):
    """The grid rows of the CG slab's cases: 0, 1, n-2, n-1 and both sides of the first and the last seam of 4-row and 8-row blocks
    (all of seam_rows would poison more than 1 % of a 129 grid)."""
    at = {0, 1, n - 2, n - 1}
    for block in (4, 8):
        seams = list(range(block, n, block))
        for s in seams[:1] + seams[-1:]:
            at |= {s - 1, s}
    return sorted(r for r in at if 0 <= r < n)


def edge_rows(n):
    """The grid rows (or planes) an operator's kernels treat differently: first two, a middle one, last two."""
    return sorted({r for r in (0, 1, n // 2, n - 2, n - 1) if 0 <= r < n})


def positions_2d(n, rows=None, cols=None):
    """(i, j) pairs that hold every column of `cols` (default seam_columns) and every row of `rows` (default edge_rows) at least
    once."""
    cols, rows = list(seam_columns(n) if cols is None else cols), list(edge_rows(n) if rows is None else rows)
    return [(rows[t % len(rows)], cols[t % len(cols)]) for t in range(max(len(cols), len(rows)))]


def positions_3d(n, cols=None):
    """(k, i, j) triples from the same lists: every seam column, every edge row and every edge plane at least once."""
    cols, rows = list(seam_columns(n) if cols is None else cols), edge_rows(n)
    return [(rows[(t + 2) % len(rows)], rows[t % len(rows)], cols[t % len(cols)]) for t in range(max(len(cols), len(rows)))]


def flat(positions, n):
    """Row numbers of (i, j) pairs or (k, i, j) triples."""
    out = []
    for p in positions:
        r = 0
        for c in p:
            r = r * n + c
        out.append(r)
    return np.array(sorted(set(out)), dtype=np.int64)


# ---------------------------------------------------------------- matrices
def stencil_csr(n, dim, rng):
    """Sorted CSR of the n^dim (dim = 2: 5-point, 3: 7-point) stencil, every value uniform in [-3, 3) \\ (-0.25, 0.25): unsymmetric,
    and no product with a finite x can vanish or cancel a poison."""
    N = n ** dim
    r = np.arange(N, dtype=np.int64)
    j, i = r % n, (r // n) % n
    steps = [(-n, i > 0), (-1, j > 0), (0, np.ones(N, dtype=bool)), (1, j < n - 1), (n, i < n - 1)]
    if dim == 3:
        k = r // (n * n)
        steps = [(-n * n, k > 0)] + steps + [(n * n, k < n - 1)]
    present = np.stack([ok for _, ok in steps], axis=1)
    cols = np.stack([r + d for d, _ in steps], axis=1)
    rp = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.int32)
    ci = cols[present].astype(np.int32)
    va = rng.uniform(0.25, 3.0, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    return rp, ci, va


def symmetrise(rp, ci, va):
    """The upper triangle's value in both directions of every edge: bitwise symmetric (a CG slab keeps its planes)."""
    rows = row_of_entry(rp)
    key = np.minimum(rows, ci).astype(np.int64) * (len(rp) - 1) + np.maximum(rows, ci)
    order = np.argsort(key, kind="stable")  # the two directions of an edge become neighbours, the upper (smaller row) first
    out = va.copy()
    k = key[order]
    second = np.flatnonzero(k[1:] == k[:-1]) + 1
    out[order[second]] = va[order[second - 1]]
    return out


def row_of_entry(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def entries_of(rp, ci, va):
    """The CSR as COO entries (what HostMatrix takes), in CSR order."""
    e = np.zeros(len(ci), dtype=ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = row_of_entry(rp), ci, va
    return e


def entry_at(rp, ci, row, col):
    """Index of entry (row, col) in the CSR arrays."""
    lo, hi = int(rp[row]), int(rp[row + 1])
    k = np.flatnonzero(ci[lo:hi] == col)
    assert len(k) == 1, (row, col)
    return lo + int(k[0])


# ---------------------------------------------------------------- planters
def x_inf(x, rows):
    """+inf in x at `rows`. Returns the poisoned copy and the positions."""
    out = np.array(x, dtype=np.float64)
    out[rows] = np.inf
    return out, np.asarray(rows, dtype=np.int64)


def x_negzero(va, x, n, i, dim=2):
    """-0.0 in x over the whole grid rows i-1 .. i+1 (dim = 3: planes) and every coefficient made positive: every product of grid row
    (plane) i is -0.0. Returns the coefficients, the poisoned x and the positions."""
    width = n ** (dim - 1)
    out = np.array(x, dtype=np.float64)
    at = np.arange((i - 1) * width, (i + 2) * width, dtype=np.int64)
    out[at] = -0.0
    return np.abs(va), out, at


def coef_targets(rp, ci, n, dim=2, clamp_targets=True):
    """Entry indices for coef_inf, all off the diagonal but the first two:
    - values[0] and values[nnz-1], where every clamped coefficient run lands (clamp_targets False leaves them out);
    - the entry in front of a grid row's first entry: what the run of that grid row's first tile holds in strip slot 0;
    - two grid rows further on, a grid row's first entry: what a short last tile's run reads on into;
    - a W or an E entry (alternating) at every seam column, each in a grid row of its own where the grid has that many."""
    nnz, width = len(ci), n ** (dim - 1)
    at = {0, nnz - 1} if clamp_targets else set()
    mid = (width // 2) * n  # column 0 of a grid row in the middle of the grid (dim = 3: of the middle plane)
    at |= {int(rp[mid]) - 1, int(rp[mid + 2 * n])}  # two grid rows apart: neither row that holds one can see the other
    for t, j in enumerate(seam_columns(n)):
        gr = (2 + t) % width if dim == 2 else (n * n // 2 + 2 + t) % width  # grid row index among the n^(dim-1) grid rows
        row = gr * n + j
        west = (t % 2 == 0 and j > 0) or j == n - 1
        at.add(entry_at(rp, ci, row, row - 1 if west else row + 1))
    return np.array(sorted(at), dtype=np.int64)


def coef_inf(rp, ci, va, targets, symmetric=False):
    """+inf in the stored coefficients at `targets`; symmetric: also in the other direction of each edge. Returns the poisoned copy
    and the positions."""
    at = set(int(t) for t in targets)
    if symmetric:
        rows = row_of_entry(rp)
        at |= {entry_at(rp, ci, int(ci[t]), int(rows[t])) for t in targets}
    at = np.array(sorted(at), dtype=np.int64)
    out = np.array(va, dtype=np.float64)
    out[at] = np.inf
    return out, at


def poisoned_rows(rp, ci, x_at, coef_at):
    """The rows that may see the poison: those whose CSR row holds a poisoned column or a poisoned coefficient."""
    hit = np.isin(ci, x_at)
    hit[np.asarray(coef_at, dtype=np.int64)] = True
    return np.unique(row_of_entry(rp)[hit])


# ---------------------------------------------------------------- the table
System = collections.namedtuple("System", "n dim planter rp ci va x x_at coef_at seams")
# seams: what the case promises to hold: ("columns", [...]) / ("rows", [...]) / ("planes", [...]) of the poisoned x positions, or
# ("entries", [...]) of the poisoned coefficients


def _seams_of(positions):
    names = ("rows", "columns") if len(positions[0]) == 2 else ("planes", "rows", "columns")
    return {name: sorted({p[a] for p in positions}) for a, name in enumerate(names)}


@functools.lru_cache(maxsize=4)
def _base(n, dim):
    rng = np.random.default_rng(9000 + 10 * n + dim)
    rp, ci, va = stencil_csr(n, dim, rng)
    x = rng.standard_normal(n ** dim)
    x[x == 0.0] = 1.0
    for a in (rp, ci, va, x):
        a.setflags(write=False)
    return rp, ci, va, x


@functools.lru_cache(maxsize=6)
def system(n, planter, dim=2, clamp_targets=True):
    """One poisoned system of the table: built once, shared, never written."""
    rp, ci, va, x = _base(n, dim)
    none = np.zeros(0, dtype=np.int64)
    if planter in ("x_inf", "x_inf_pairs"):
        cols = pair_columns(n) if planter == "x_inf_pairs" else None
        positions = positions_2d(n, cols=cols) if dim == 2 else positions_3d(n, cols)
        xp, x_at = x_inf(x, flat(positions, n))
        s = System(n, dim, planter, rp, ci, va, xp, x_at, none, _seams_of(positions))
    elif planter == "x_negzero":
        i = n // 2
        vp, xp, x_at = x_negzero(va, x, n, i, dim)
        s = System(n, dim, planter, rp, ci, vp, xp, x_at, none, {"rows" if dim == 2 else "planes": [i - 1, i, i + 1]})
    elif planter == "coef_inf":
        targets = coef_targets(rp, ci, n, dim, clamp_targets)
        vp, coef_at = coef_inf(rp, ci, va, targets)
        s = System(n, dim, planter, rp, ci, vp, x, none, coef_at, {"entries": targets.tolist()})
    else:
        raise KeyError(planter)
    for a in (s.va, s.x, s.x_at, s.coef_at):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=4)
def slab_system(n, planter):
    """The single-rank CG slab's poisoned system: bitwise symmetric (the slab keeps its planes), diagonal positive (A 0 is +0.0 on
    every row, so b can serve as p0); +inf in x at the seam columns of slab_rows, or in both directions of coef_targets' edges."""
    rp, ci, va, x = _base(n, 2)
    va = symmetrise(rp, ci, va)
    diagonal = row_of_entry(rp) == ci
    va[diagonal] = np.abs(va[diagonal])
    none = np.zeros(0, dtype=np.int64)
    if planter == "x_inf":
        positions = positions_2d(n, slab_rows(n))
        xp, x_at = x_inf(x, flat(positions, n))
        s = System(n, 2, planter, rp, ci, va, xp, x_at, none, _seams_of(positions))
    else:
        assert planter == "coef_inf"
        targets = coef_targets(rp, ci, n)
        vp, coef_at = coef_inf(rp, ci, va, targets, symmetric=True)
        s = System(n, 2, planter, rp, ci, vp, x, none, coef_at, {"entries": targets.tolist()})
    for a in (s.va, s.x, s.x_at, s.coef_at):
        a.setflags(write=False)
    return s


SLAB_TABLE = [(n, planter) for n in GRIDS_2D for planter in ("x_inf", "coef_inf")]
TABLE = [(n, planter, 2, True) for n in GRIDS_2D for planter in PLANTERS] + [(n, "coef_inf", 2, False) for n in GRIDS_2D] + \
        [(n, planter, 3, True) for n in GRIDS_3D for planter in PLANTERS] + \
        [(n, "x_inf_pairs", d, True) for d, grids in ((2, (9, 129, 257)), (3, (65, 129))) for n in grids]  # the transfers' odd grids


# ---------------------------------------------------------------- the cases that are no plain stencil system
UNIFORM_TABLE = [(name, planter) for name in ("aniso-129", "aniso-257") for planter in ("x_inf", "coef_inf")]


@functools.lru_cache(maxsize=4)
def uniform_system(name, planter):
    """An anisotropic stencil of tests/layered.py (every tile of grid rows 1 .. n-2 is uniform) with the poison inside a uniform tile:
    +inf in x at the seam columns of slab_rows, or in both directions of one horizontal edge inside the first column tile (columns
    63 | 64 of a grid row below the middle). seams["tile"]: the (grid row, column tile) a poisoned coefficient makes class 0."""
    import layered
    from oracle import oracle as O

    n, _, rp, ci, va = layered.case(O, name)
    x = np.random.default_rng(4600 + n).standard_normal(n * n)
    none = np.zeros(0, dtype=np.int64)
    if planter == "x_inf":
        positions = positions_2d(n, slab_rows(n))
        xp, x_at = x_inf(x, flat(positions, n))
        s = System(n, 2, planter, rp, ci, va, xp, x_at, none, _seams_of(positions))
    else:
        assert planter == "coef_inf"
        gi = n // 2 + 1
        targets = np.array([entry_at(rp, ci, gi * n + 63, gi * n + 64)])
        vp, coef_at = coef_inf(rp, ci, va, targets, symmetric=True)
        s = System(n, 2, planter, rp, ci, vp, x, none, coef_at, {"entries": targets.tolist(), "tile": (gi, 0)})
    for a in (s.va, s.x, s.x_at, s.coef_at):
        a.setflags(write=False)
    return s


def padding_case():
    """(entries, rows, cols, x): ragged rows (some empty), none with an entry in column 0 or in the last column, and +inf in x at
    both: only a padding slot of an ELLPACK row could reach them."""
    import matrices

    e, rows, cols = matrices.random_sparse(300, 500, lambda row, rng: 0 if row % 11 == 0 else int(rng.integers(1, 9)), seed=23)
    e = e[(e["col"] != 0) & (e["col"] != cols - 1)]
    x = np.random.default_rng(24).standard_normal(cols)
    x[0] = x[cols - 1] = np.inf
    return e, rows, cols, x


CHEBYSHEV_CASES = ("r", "dinv", "coefficient")
CHEBYSHEV_BOUNDS = (0.1, 3.0)  # explicit: no Gershgorin pass over a poisoned matrix


@functools.lru_cache(maxsize=4)
def chebyshev_system(n, case):
    """The fused Chebyshev step's inputs through an application z = M^-1 r (term 0: z0 = d0 = c0 dinv r, then `degree` fused steps,
    each reading z through the tile's W / E / N / S paths and r, d and dinv at its own row), on the stencil of the table with its
    diagonal made positive (creation wants one sign). Returns a System whose x is r:
    "r"            +inf in r at the seam positions: z0 and d0 hold it at the same places, so the first step meets it in z, r and d;
    "dinv"         the smallest subnormal on the diagonal there: dinv = 1 / d is +inf, r is finite, z0 and d0 hold inf again;
    "coefficient"  +inf in off-diagonal coefficients (coef_targets without the first and last entry of the matrix, which are
                   diagonal entries: creation refuses a diagonal that is not finite).
    After one step the non-finite rows of z are poisoned_rows (tests/test_poison_host.py)."""
    rp, ci, va, x = _base(n, 2)
    diagonal = row_of_entry(rp) == ci
    va = np.array(va)
    va[diagonal] = np.abs(va[diagonal])
    at = flat(positions_2d(n), n)
    none = np.zeros(0, dtype=np.int64)
    if case == "r":
        r, _ = x_inf(x, at)
        s = System(n, 2, case, rp, ci, va, r, at, none, {})
    elif case == "dinv":
        va[np.flatnonzero(diagonal)[at]] = 5e-324
        s = System(n, 2, case, rp, ci, va, np.array(x), at, none, {})
    else:
        assert case == "coefficient"
        va, coef_at = coef_inf(rp, ci, va, coef_targets(rp, ci, n, 2, clamp_targets=False))
        s = System(n, 2, case, rp, ci, va, np.array(x), none, coef_at, {})
    for a in (s.va, s.x, s.x_at, s.coef_at):
        a.setflags(write=False)
    return s
