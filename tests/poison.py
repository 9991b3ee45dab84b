"""Poisoned inputs for the stencil kernels (tests/test_poison_host.py, tests/test_poison_gpu.py) and, in the section "general CSR" at
the end, for the AMG transfers and the CSR family (tests/test_poison_csr_host.py, tests/test_poison_csr_gpu.py). Test infrastructure
only.

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


# ================================================================ general CSR: the AMG transfers and the CSR family
# (tests/test_poison_csr_host.py, tests/test_poison_csr_gpu.py)
#
# amg_residual_restrict_kernel and its batched form (csrc/amg.hip, csrc/amg_multi.hip) give eight lanes to an aggregate and eight
# aggregates to a wave; the round count is the wave's maximum, so a group that is done keeps shuffling with `have <= 0`. The seams are
# between the members of one round, between rounds, between the eight groups of a wave and between waves. Aggregate I is group I % 8
# of wave I // 8.
AGG_WAVES = (
    [100, 1, 1, 1, 1, 1, 1, 1],       # 13 rounds in group 0; the seven singles sit at have <= 0 for twelve of them
    [1, 7, 8, 9, 16, 17, 2, 100],     # the long aggregate in the last group; sizes around one and two rounds
    [8] * 8,                          # a full wave of full single rounds
    [9, 1, 17, 3, 8],                 # a last wave with three dead groups (live == false)
)
AGG_TARGETS = ((0, 0), (0, 1), (1, 7), (2, 0), (3, 4), (1, 3))  # (wave, group)
AGG_PLANTERS = ("r_inf", "z_inf", "coef_inf", "negzero_sum", "negzero_chain")
AGG_POOL = 2000      # the common columns [0, 2000); the reserved band lies behind them
AGG_SEED = 2900

AggLevel = collections.namedtuple("AggLevel", "rp ci va count agg agg_ptr members z r cols reserved free_rows")
AggCase = collections.namedtuple("AggCase", "planter target slot rp ci va z r rows_at planted touched")
# rows_at: the fine rows the poison was planted at; planted: the coarse rows that may be non-finite; touched: the coarse rows whose
# inputs differ from the clean level's (every other coarse row must come out with the clean run's bits)


def coarse_of(target):
    return 8 * target[0] + target[1]


@functools.lru_cache(maxsize=1)
def aggregate_level():
    """One level for the restriction: 29 aggregates of AGG_WAVES' sizes, members dealt at random and ascending inside each aggregate,
    five more rows owned by nobody. Rows hold 0, 1, 5 or 70 entries with values in U(0.25, 3); the members at slots 0, 7, 8 and last
    of every target aggregate hold 5, 70, 1 and 5 (a later slot wins where two coincide), so a poison can be planted there. Columns
    come from the pool [0, 2000); every non-empty member row of a target aggregate also holds, as its last entry, a reserved column of
    its own behind the pool that no other row refers to (reserved[row], else -1): poison in z there reaches that row alone. z and r are
    standard normal, z nowhere zero. Built once, never written."""
    rng = np.random.default_rng(AGG_SEED)
    sizes = np.array([s for wave in AGG_WAVES for s in wave], dtype=np.int64)
    count, owned = len(sizes), int(sizes.sum())
    rows = owned + 5
    deal = rng.permutation(rows)
    free_rows, deal = np.sort(deal[:5]), deal[5:]
    agg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = np.concatenate([np.sort(deal[agg_ptr[I]:agg_ptr[I + 1]]) for I in range(count)]).astype(np.int32)
    agg = np.full(rows, -1, dtype=np.int32)
    agg[members] = np.repeat(np.arange(count), sizes)
    lengths = rng.choice([0, 1, 5, 70], size=rows, p=[0.15, 0.15, 0.6, 0.1])
    reserved = np.full(rows, -1, dtype=np.int64)
    band = AGG_POOL
    for target in AGG_TARGETS:
        m = members[agg_ptr[coarse_of(target)]:agg_ptr[coarse_of(target) + 1]]
        for slot, n in ((0, 5), (7, 70), (8, 1), (len(m) - 1, 5)):
            if slot < len(m):
                lengths[m[slot]] = n
        for row in m[lengths[m] > 0]:
            reserved[row], band = band, band + 1
    cols = band
    body = []
    for row in range(rows):
        n = int(lengths[row])
        own = [reserved[row]] if reserved[row] >= 0 else []
        body.append(np.concatenate([np.sort(rng.choice(AGG_POOL, size=n - len(own), replace=False)), own]))
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate(body).astype(np.int32)
    va = rng.uniform(0.25, 3.0, len(ci))
    z, r = rng.standard_normal(cols), rng.standard_normal(rows)
    z[z == 0.0] = 1.0
    for a in (rp, ci, va, agg, agg_ptr, members, z, r, reserved, free_rows):
        a.setflags(write=False)
    return AggLevel(rp, ci, va, count, agg, agg_ptr, members, z, r, cols, reserved, free_rows)


def target_members(target, level=None):
    L = aggregate_level() if level is None else level
    I = coarse_of(target)
    return L.members[L.agg_ptr[I]:L.agg_ptr[I + 1]].astype(np.int64)


def target_slots(target):
    """The positions inside a target: "all" (the whole aggregate), and one member at slot 0, 7, 8 or last, each once."""
    size = len(target_members(target))
    singles = sorted({s for s in (0, 7, 8, size - 1) if s < size})
    return (["all"] if size > 1 else []) + singles


def planted_coarse(rp, ci, va, z, r, agg_ptr, members):
    """The coarse rows that may be non-finite, by plain indexing: aggregate I is in iff one of its member rows holds a non-finite r, a
    non-finite stored value, or a column at which z is not finite."""
    entry_hit = ~np.isfinite(va) | ~np.isfinite(z[ci])
    row_hit = ~np.isfinite(r)
    row_hit[row_of_entry(rp)[entry_hit]] = True
    return np.array([I for I in range(len(agg_ptr) - 1) if row_hit[members[agg_ptr[I]:agg_ptr[I + 1]]].any()], dtype=np.int64)


def _emptied(L, rows):
    """The level's CSR with `rows` left without entries."""
    keep = ~np.isin(row_of_entry(L.rp), rows)
    lengths = np.diff(L.rp).astype(np.int64)
    lengths[rows] = 0
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), L.ci[keep].copy(), L.va[keep].copy()


@functools.lru_cache(maxsize=None)
def aggregate_case(planter, target, slot):
    """One poisoned form of aggregate_level(), built once, never written.
    r_inf          +inf in r at the chosen member rows: r_c = +inf at the target
    z_inf          +inf in z at the chosen rows' reserved columns: the coefficients are positive, so r_c = -inf
    coef_inf       +inf in one stored value of each chosen row: a non-finite r_c
    negzero_sum    every member of the target has an empty row and r = -0.0: r_c is -0.0, a sum started at +0.0 gives +0.0
    negzero_chain  the member at `slot` keeps its row, z = -0.0 at its columns and r = -0.0 there: its chain starts at +0.0, so its
                   t = fma(-1.0, +0.0, -0.0) is -0.0, where a chain started from its first product gives +0.0; every other member is
                   as in negzero_sum, so that one t decides the sign of r_c
    "all" chooses every member (z_inf and coef_inf: every member that has an entry)."""
    L = aggregate_level()
    m = target_members(target)
    I = coarse_of(target)
    rp, ci, va, z, r = L.rp, L.ci, L.va.copy(), L.z.copy(), L.r.copy()
    chosen = m if slot == "all" else m[[slot]]
    touched = {I}
    if planter == "r_inf":
        r[chosen] = np.inf
    elif planter in ("z_inf", "coef_inf"):
        chosen = chosen[np.diff(rp)[chosen] > 0]
        assert len(chosen) > 0 and (L.reserved[chosen] >= 0).all(), (target, slot)
        if planter == "z_inf":
            z[L.reserved[chosen]] = np.inf
        else:
            va[rp[chosen] + chosen % np.diff(rp)[chosen]] = np.inf
    elif planter == "negzero_sum":
        assert slot == "all"
        rp, ci, va = _emptied(L, m)
        r[m] = -0.0
    elif planter == "negzero_chain":
        assert slot != "all" and rp[chosen[0] + 1] > rp[chosen[0]]
        rp, ci, va = _emptied(L, m[m != chosen[0]])
        r[m] = -0.0
        at = ci[rp[chosen[0]]:rp[chosen[0] + 1]]
        z[at] = -0.0
        holders = np.unique(row_of_entry(rp)[np.isin(ci, at)])
        touched |= {int(a) for a in L.agg[holders] if a >= 0}
    else:
        raise KeyError(planter)
    planted = planted_coarse(rp, ci, va, z, r, L.agg_ptr, L.members)
    for a in (rp, ci, va, z, r, planted):
        a.setflags(write=False)
    return AggCase(planter, target, slot, rp, ci, va, z, r, chosen, planted, np.array(sorted(touched), dtype=np.int64))


def aggregate_cases(planter):
    """Every (planter, target, slot) of the table: the inf planters at every slot of every target, negzero_sum on whole targets,
    negzero_chain at the single slots."""
    out = []
    for target in AGG_TARGETS:
        slots = target_slots(target)
        if planter == "negzero_sum":
            slots = ["all"]
        elif planter == "negzero_chain":
            slots = [s for s in slots if s != "all"]
        out += [(planter, target, s) for s in slots]
    return out


AGG_TABLE = [c for planter in AGG_PLANTERS for c in aggregate_cases(planter)]


@functools.lru_cache(maxsize=None)
def aggregate_reference(planter=None, target=None, slot=None):
    """r_c = restrict(r - A z) of a case (no planter: of the clean level): the oracle's sequential chain, its fma for the residual,
    amg_restatement.restrict for the sum over the members from the first member's t. Computed once, shared, never written."""
    import amg_restatement as AMG
    from oracle import oracle as O

    L = aggregate_level()
    c = L if planter is None else aggregate_case(planter, target, slot)
    with np.errstate(invalid="ignore"):
        t = O.axpy(-1.0, O.spmv_csr(c.rp, c.ci, c.va, c.z), c.r)
        out = AMG.restrict(t, AMG.Aggregates(L.count, L.agg, L.agg_ptr, L.members))
    out.setflags(write=False)
    return out


# ---- the prolongation
PROLONG_ROWS = (1, 2, 3, 129, 4225)
ProlongLevel = collections.namedtuple("ProlongLevel", "rows coarse_rows agg z ec")


@functools.lru_cache(maxsize=None)
def prolong_level(rows):
    """agg deals the rows to max(1, min(rows, max(2, rows // 4))) aggregates at random, none empty; rows 0 and 1 -- one 16-byte pair
    -- lie in different aggregates wherever there are two rows (at 129 and 4 225 most pairs do); an odd `rows` leaves the last row
    outside every pair. z and e_c standard normal."""
    rng = np.random.default_rng(7100 + rows)
    coarse_rows = max(1, min(rows, max(2, rows // 4)))
    agg = rng.permutation(np.arange(rows) % coarse_rows).astype(np.int32)
    if rows > 1 and agg[0] == agg[1]:
        other = int(np.flatnonzero(agg != agg[0])[0])
        agg[1], agg[other] = agg[other], agg[1]
    z, ec = rng.standard_normal(rows), rng.standard_normal(coarse_rows)
    for a in (agg, z, ec):
        a.setflags(write=False)
    return ProlongLevel(rows, coarse_rows, agg, z, ec)


def prolong_cases(rows):
    """(label, e_c, z, I): +inf in e_c at aggregate I = 0, a middle one and the last one (each once), and the -0.0 case (I None):
    e_c = -0.0 and z = -0.0 everywhere give -0.0 everywhere."""
    L = prolong_level(rows)
    out = []
    for I in sorted({0, L.coarse_rows // 2, L.coarse_rows - 1}):
        ec = L.ec.copy()
        ec[I] = np.inf
        out.append((f"inf@{I}", ec, L.z, I))
    out.append(("negzero", np.full(L.coarse_rows, -0.0), np.full(rows, -0.0), None))
    return out


# ---- two CSR matrices as a file gives them: sorted rows in which equal columns stay adjacent in input order
def _poisson(n):
    rp, ci, _ = stencil_csr(n, 2, np.random.default_rng(0))
    return rp, ci, np.where(row_of_entry(rp) == ci, 4.0, -1.0)


def _with_twins(rp, ci, va, first, second):
    """Entry k stays alone where second[k] is NaN, else becomes the adjacent pair (first[k], second[k]) in its column."""
    pair = ~np.isnan(second)
    copies = np.where(pair, 2, 1)
    src = np.repeat(np.arange(len(ci)), copies)
    is_second = np.concatenate([[False], src[1:] == src[:-1]])
    values = np.where(is_second, second[src], first[src])
    lengths = np.bincount(row_of_entry(rp)[src], minlength=len(rp) - 1)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), ci[src].astype(np.int32), values


@functools.lru_cache(maxsize=1)
def split33():
    """The 33 x 33 Poisson matrix with each entry v in one of three forms chosen at random: kept; split into v / 4 and 3 v / 4 (both
    exact in fp64, as is their sum); given a stored 0.0 twin, in front of it or behind it. The summed matrix is Poisson: symmetric
    positive definite. Returns (rp, ci, va), built once, never written."""
    rng = np.random.default_rng(3301)
    rp, ci, va = _poisson(33)
    form = rng.integers(0, 3, len(ci))
    zero_first = rng.random(len(ci)) < 0.5
    first = np.where(form == 1, va / 4.0, np.where((form == 2) & zero_first, 0.0, va))
    second = np.where(form == 1, 3.0 * va / 4.0, np.where(form == 2, np.where(zero_first, va, 0.0), np.nan))
    out = _with_twins(rp, ci, va, first, second)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def oneway33():
    """split33 with about a tenth of its lone entries v turned into the partly cancelling pair (3 v, -2 v), and about 7 % of the
    edges i < j left with one direction only (every stored part of the other goes). The pattern is not symmetric; every row stays
    weakly diagonally dominant with its diagonal 4. Returns (rp, ci, va), built once, never written."""
    rng = np.random.default_rng(3302)
    rp, ci, va = split33()
    rows = row_of_entry(rp)
    n = len(rp) - 1
    key = rows * n + ci
    lone = np.ones(len(ci), dtype=bool)
    lone[1:] &= key[1:] != key[:-1]
    lone[:-1] &= key[1:] != key[:-1]
    cancel = lone & (rng.random(len(ci)) < 0.1)
    first, second = np.where(cancel, 3.0 * va, va), np.where(cancel, -2.0 * va, np.nan)
    rp, ci, va = _with_twins(rp, ci, va, first, second)
    rows = row_of_entry(rp)
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)
    edges = np.unique((lo * n + hi)[rows != ci])
    gone = edges[rng.random(len(edges)) < 0.07]
    upper = rng.random(len(gone)) < 0.5            # which direction of the edge goes
    gone_key = np.where(upper, (gone // n) * n + gone % n, (gone % n) * n + gone // n)
    keep = ~np.isin(rows * n + ci, gone_key)
    lengths = np.bincount(rows[keep], minlength=n)
    out = (np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), ci[keep].copy(), va[keep].copy())
    for a in out:
        a.setflags(write=False)
    return out


def shuffled_entries(rp, ci, va, seed):
    """The CSR as COO entries in a random order: what a file with its lines shuffled gives."""
    e = entries_of(rp, ci, va)
    return e[np.random.default_rng(seed).permutation(len(e))]


def csr_of_entries(e, rows):
    """What build_csr_struct makes of COO entries: rows ascending, columns ascending inside a row, equal columns in input order."""
    order = np.lexsort((e["col"], e["row"]))  # stable: ties keep the input order
    rp = np.concatenate([[0], np.cumsum(np.bincount(e["row"], minlength=rows))]).astype(np.int32)
    return rp, e["col"][order].astype(np.int32), np.ascontiguousarray(e["value"][order], dtype=np.float64)
