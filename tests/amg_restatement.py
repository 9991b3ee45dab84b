"""numpy restatement of the aggregation AMG preconditioner of csrc/amg.hip and csrc/amg_setup.hpp, written
from the text of include/spmv_amd/api.h under spmv_amd_precond_create_amg and not from outputs: the diagonal, the strong couplings,
the three aggregation passes, the member lists, the Galerkin sums in their stated order, the per-level intervals, and the V-cycle in
two forms -- plain numpy (two roundings per a * b + c, products in scipy's order) and exact (every level's product through
csr_restatement's row sums in that level's variant, the restriction's residual through the sequential chain, every update the
oracle's fma) --, the preconditioned loops in two roundings and in the device's bits, and the systems of the whole-solve table, made
with numpy only and seeded."""
import collections
import functools

import numpy as np
import scipy.sparse as sp

import chebyshev_restatement as CH
import csr_restatement as CSR
import reduction_restatement as RR

THETA = 0.08
COARSEST_ROWS = 64
MAX_LEVELS = 32
COARSEST_DEGREE = 8
FINE_RATIO = 4.0
COARSEST_RATIO = 30.0

Csr = collections.namedtuple("Csr", "rp ci va")
Aggregates = collections.namedtuple("Aggregates", "count agg agg_ptr members")


def csr_of(A):
    """A scipy matrix as sorted CSR arrays (stored zeros kept): what cusparse-csr holds."""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return Csr(A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data, dtype=np.float64))


def scipy_of(M):
    n = len(M.rp) - 1
    return sp.csr_matrix((M.va, M.ci, M.rp), shape=(n, n))


def rows_of(M):
    return len(M.rp) - 1


def row_index(M):
    return np.repeat(np.arange(rows_of(M)), np.diff(M.rp))


def diagonal(M):
    """d_i = the sum of row i's entries in column i, CSR order, from 0.0 (np.add.at adds one entry at a time, in order)."""
    d = np.zeros(rows_of(M))
    on = np.nonzero(M.ci == row_index(M))[0]
    np.add.at(d, row_index(M)[on], M.va[on])
    return d


def strong_mask(M, theta):
    """Entry k of row i, column j != i, value v: strong iff v * v > t2 * fabs(d_i * d_j), t2 = theta * theta."""
    d, row = diagonal(M), row_index(M)
    t2 = theta * theta
    return (M.ci != row) & (M.va * M.va > t2 * np.abs(d[row] * d[M.ci]))


def aggregate(M, theta=THETA):
    """The three passes in ascending row order; aggregates numbered in order of creation; members ascending."""
    n = rows_of(M)
    mask = strong_mask(M, theta)
    row = row_index(M)
    sptr = np.concatenate([[0], np.cumsum(np.bincount(row[mask], minlength=n))])
    scol = M.ci[mask].tolist()
    strong = [scol[sptr[i]:sptr[i + 1]] for i in range(n)]
    agg = [-1] * n
    count = 0
    for i in range(n):  # pass 1
        if agg[i] >= 0 or any(agg[j] >= 0 for j in strong[i]):
            continue
        agg[i] = count
        for j in strong[i]:
            agg[j] = count
        count += 1
    first = list(agg)
    for i in range(n):  # pass 2, from the copy
        if first[i] >= 0:
            continue
        for j in strong[i]:
            if first[j] >= 0:
                agg[i] = first[j]
                break
    for i in range(n):  # pass 3
        if agg[i] >= 0:
            continue
        agg[i] = count
        for j in strong[i]:
            if agg[j] < 0:
                agg[j] = count
        count += 1
    agg = np.array(agg, dtype=np.int32)
    members = np.argsort(agg, kind="stable").astype(np.int32)
    agg_ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=count))]).astype(np.int32)
    return Aggregates(count, agg, agg_ptr, members)


def sums_in_order(keys, values, size):
    """Per key the plain sequential sum of its values in the order given, starting from the key's first value (not from 0.0). Every
    key of range(size) must occur."""
    out = np.zeros(size)
    _, first = np.unique(keys, return_index=True)
    assert len(first) == size
    out[keys[first]] = values[first]
    rest = np.ones(len(keys), dtype=bool)
    rest[first] = False
    np.add.at(out, keys[rest], values[rest])
    return out


def galerkin(M, g):
    """A_c = P^T A P: the members of I in ascending order, each member's entries in CSR order; one entry per distinct J = agg(col),
    sorted by J, stored zeros kept."""
    lengths = np.diff(M.rp)[g.members]
    start = M.rp[:-1][g.members].astype(np.int64)
    # the fine entries in the order the coarse rows walk them
    offsets = np.arange(int(lengths.sum())) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    at = np.repeat(start, lengths) + offsets
    I = np.repeat(g.agg[g.members].astype(np.int64), lengths)
    J = g.agg[M.ci[at]].astype(np.int64)
    key = I * g.count + J
    uniq, inv = np.unique(key, return_inverse=True)  # ascending (I, J): CSR order of the coarse matrix
    values = sums_in_order(inv.ravel(), M.va[at], len(uniq))
    rp = np.concatenate([[0], np.cumsum(np.bincount(uniq // g.count, minlength=g.count))]).astype(np.int32)
    return Csr(rp, (uniq % g.count).astype(np.int32), values)


def structure(M, max_levels=0, theta=THETA):
    """[(matrix, aggregates or None)]: the levels before any interval is known. Level l is the coarsest if rows <= 64, if
    l + 1 == max_levels (0: 32), or if its aggregation gives 10 n_c > 9 rows (discarded)."""
    out = []
    while True:
        rows, l = rows_of(M), len(out)
        g = None
        if not (rows <= COARSEST_ROWS or l + 1 == (max_levels if max_levels > 0 else MAX_LEVELS)):
            g = aggregate(M, theta)
            if 10 * g.count > 9 * rows:
                g = None
        out.append((M, g))
        if g is None:
            return out
        M = galerkin(M, g)


class Level:
    def __init__(self, M, g, dinv, lambda_max, coef):
        self.M, self.g, self.dinv, self.lambda_max, self.coef = M, g, dinv, lambda_max, coef
        self.A = scipy_of(M)
        self.rows = rows_of(M)


def hierarchy(M, nu, max_levels=0, theta=THETA, levels=None):
    """The levels with dinv, the symmetric Gershgorin bound and the coefficients. levels: a structure() made before (it does not
    depend on nu)."""
    levels = structure(M, max_levels, theta) if levels is None else levels
    out = []
    for l, (Ml, g) in enumerate(levels):
        with np.errstate(divide="ignore"):
            dinv = 1.0 / diagonal(Ml)
        hi = CH.gershgorin(scipy_of(Ml), dinv)
        last = l == len(levels) - 1
        lo = hi / COARSEST_RATIO if last else hi / FINE_RATIO
        out.append(Level(Ml, g, dinv, hi, CH.coefficients(COARSEST_DEGREE if last else nu, lo, hi)))
    return out


def restrict(t, g):
    """r_c[I] = ((t_m0 + t_m1) + t_m2) + ... over the members in ascending order."""
    return sums_in_order(g.agg[g.members].astype(np.int64), t[g.members], g.count)


def make_cycle(levels, matvecs=None, chains=None, fma=None):
    """r -> z = M^-1 r, one V-cycle. matvecs[l]: level l's product as its smoother runs it; chains[l]: the product the restriction's
    residual uses (the sequential chain on every level); both default to A_l @ v. fma(a, x, y) = a * x + y rounded once (the
    oracle's axpy); None: two roundings."""
    if fma is None:
        def fma(a, x, y):
            return a * x + y
    if matvecs is None:
        matvecs = [(lambda v, A=L.A: A @ v) for L in levels]
    if chains is None:
        chains = matvecs

    def update(L, mv, r, d, z, g, h):
        t = fma(-1.0, mv(z), r)
        u = L.dinv * t
        d = fma(g, u, h * d)
        return d, z + d

    def cycle(l, r):
        L, mv = levels[l], matvecs[l]
        degree = (len(L.coef) - 1) // 2
        d = L.coef[0] * (L.dinv * r)
        z = d.copy()
        for k in range(1, degree + 1):
            d, z = update(L, mv, r, d, z, L.coef[2 * k], L.coef[2 * k - 1])
        if l == len(levels) - 1:
            return z
        rc = restrict(fma(-1.0, chains[l](z), r), L.g)
        ec = cycle(l + 1, rc)
        z = fma(2.0, ec[L.g.agg], z)
        d, z = update(L, mv, r, d, z, L.coef[0], 0.0)
        for k in range(1, degree + 1):
            d, z = update(L, mv, r, d, z, L.coef[2 * k], L.coef[2 * k - 1])
        return z

    return lambda r: cycle(0, r)


def exact_products(O, levels, variant0=None):
    """(matvecs, chains) of the device: level 0 in the operator's variant (None: the automatic one), every other level in the
    automatic variant of its matrix; the chains are the sequential sum on every level."""
    matvecs, chains = [], []
    for l, L in enumerate(levels):
        variant = CSR.variant_of(L.M.rp, variant0 if l == 0 else None)
        matvecs.append(lambda v, M=L.M, variant=variant: CSR.row_sums(M.rp, M.ci, M.va, v, variant))
        chains.append(lambda v, M=L.M: O.spmv_csr(M.rp, M.ci, M.va, v))
    return matvecs, chains


def exact_cycle(O, levels, variant0=None):
    matvecs, chains = exact_products(O, levels, variant0)
    return make_cycle(levels, matvecs, chains, fma=O.axpy)


def other_cycle(levels):
    """The cycle with every product through the level's CSC form."""
    forms = [sp.csc_matrix(L.A) for L in levels]
    return make_cycle(levels, [(lambda v, T=T: T @ v) for T in forms])


def long_dot(u, v):
    ld = np.longdouble
    return float(np.sum(u.astype(ld) * v.astype(ld)))


def pcg(levels, b, x0, tol=1e-6, max_iters=1000):
    """AMG-PCG in plain numpy. Returns x, history, iterations, converged."""
    A = levels[0].A
    return CH._loop(lambda v: A @ v, lambda u, v: float(u @ v), b, x0, make_cycle(levels), tol, max_iters)


def pcg_other_rounding(levels, b, x0, tol=1e-6, max_iters=1000):
    T = sp.csc_matrix(levels[0].A)
    return CH._loop(lambda v: T @ v, long_dot, b, x0, other_cycle(levels), tol, max_iters)


def jacobi_pcg(M, b, x0, tol=1e-6, max_iters=2000):
    import pcg_restatement as P
    return P.pcg(scipy_of(M), b, x0, 1.0 / diagonal(M), tol, max_iters)


def pcg_exact(O, M, apply, b, x0, tol=1e-6, max_iters=1000, variant0=None):
    """spmv_amd_pcg_solve_device with kind "multigrid" on cusparse-csr in the device's bits (csrc/pcg.hip: mg_first, mg_next and the
    loop around them): the operator's product in its variant; p.Ap from the fused partials of csr/stream and csr/adaptive
    (csr_restatement.stream_block_partials) or, in the other variants, from the streaming dot partials; r.r from the r update's
    partials and r.z from the last step's, both the streaming form; every sum by pcg_reduce_kernel; every update an fma. apply: the
    application in the device's bits. The converging iteration runs no cycle. Returns x, history, iterations, converged."""
    n = rows_of(M)
    variant = CSR.variant_of(M.rp, variant0)
    per_block, _ = CSR.stream_geometry(n, int(M.rp[-1]))

    def product(v):
        return CSR.row_sums(M.rp, M.ci, M.va, v, variant)

    def total(partials):
        return RR.reduce_pcg(partials, len(partials), 1)[0]

    def fma(a, u, c):
        return O.fma(np.full(n, a), u, c)

    def usable(v):
        return v != 0.0 and np.isfinite(v)

    b = np.asarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    r = b - product(x)  # fma(1.0, b, -1.0 * Ap): the difference rounded once
    b_norm = float(np.sqrt(total(RR.stream_partials(r, r))))
    hist = [b_norm]
    z = apply(r)
    rz = total(RR.stream_partials(r, z))
    p = z.copy()
    it, converged = 0, False
    for _ in range(max_iters):
        Ap = product(p)
        pAp = total(CSR.stream_block_partials(p, Ap, per_block) if variant in ("stream", "adaptive") else RR.dot_partials(p, Ap))
        it += 1
        if not usable(pAp):
            hist.append(float(np.sqrt(total(RR.stream_partials(r, r)))))
            break
        alpha = rz / pAp
        r = fma(-alpha, Ap, r)
        res = float(np.sqrt(total(RR.stream_partials(r, r))))
        hist.append(res)
        if res / b_norm < tol:
            converged = True
            x = fma(alpha, p, x)
            break
        z = apply(r)
        rzn = total(RR.stream_partials(r, z))
        x = fma(alpha, p, x)
        if not usable(rzn):
            break
        beta = rzn / rz
        rz = rzn
        p = fma(beta, p, z)
    return x, np.array(hist), it, converged


# ---------------------------------------------------------------- systems
def poisson2d(nx, ny=None, cy=1.0):
    """The 5-point Laplacian on an nx x ny grid (rows of nx points), y-coupling cy: diagonal 2 + 2 cy."""
    ny = nx if ny is None else ny
    tx = sp.diags([np.full(nx - 1, -1.0), np.full(nx, 2.0), np.full(nx - 1, -1.0)], [-1, 0, 1])
    ty = sp.diags([np.full(ny - 1, -cy), np.full(ny, 2.0 * cy), np.full(ny - 1, -cy)], [-1, 0, 1])
    return csr_of(sp.kron(sp.identity(ny), tx) + sp.kron(ty, sp.identity(nx)))


def poisson3d(n):
    t = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1])
    e = sp.identity(n)
    return csr_of(sp.kron(sp.kron(e, e), t) + sp.kron(sp.kron(e, t), e) + sp.kron(sp.kron(t, e), e))


def ninepoint(n):
    """The 9-point stencil: 8 on the diagonal, -1 to all eight neighbours."""
    band = sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])
    return csr_of(9.0 * sp.identity(n * n) - sp.kron(band, band))


def permuted(M, seed):
    """P A P^T for a random permutation."""
    n = rows_of(M)
    perm = np.random.default_rng(seed).permutation(n)
    A = scipy_of(M).tocoo()
    return csr_of(sp.csr_matrix((A.data, (perm[A.row], perm[A.col])), shape=(n, n)))


def knn_laplacian(points, k=6, seed=0, shift=1e-3):
    """The graph Laplacian of the symmetrised k-nearest-neighbour graph of `points` uniform points of the unit square (brute-force
    distances, unit weights) + shift I."""
    xy = np.random.default_rng(seed).random((points, 2))
    rows, cols = [], []
    for lo in range(0, points, 500):
        block = xy[lo:lo + 500]
        d2 = ((block[:, None, :] - xy[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(len(block)), lo + np.arange(len(block))] = np.inf
        near = np.argsort(d2, axis=1, kind="stable")[:, :k]
        rows.append(np.repeat(lo + np.arange(len(block)), k))
        cols.append(near.ravel())
    i, j = np.concatenate(rows), np.concatenate(cols)
    W = sp.csr_matrix((np.ones(len(i)), (i, j)), shape=(points, points))
    W = ((W + W.T) > 0).astype(np.float64)
    degree = np.asarray(W.sum(axis=1)).ravel()
    return csr_of(sp.diags(degree + shift) - W)


def arrow(n=3000):
    a = CSR.arrow(n)
    return Csr(a.rp, a.ci, a.va)


def as_a_file_gives_it(name):
    """split33 / oneway33 of tests/poison.py: the 33 x 33 Poisson matrix with duplicate entries, stored zeros and (oneway33) partly
    cancelling pairs and one-way entries, rows sorted, equal columns adjacent in input order. Not through csr_of: scipy would be free
    to reorder or merge the duplicates."""
    import poison
    return Csr(*getattr(poison, name)())


SYSTEMS = {
    "poisson33": lambda: poisson2d(33), "poisson64": lambda: poisson2d(64), "poisson127": lambda: poisson2d(127),
    "permuted33": lambda: permuted(poisson2d(33), 33), "permuted64": lambda: permuted(poisson2d(64), 64),
    "aniso64": lambda: poisson2d(64, cy=0.01),
    "cube9": lambda: poisson3d(9), "cube16": lambda: poisson3d(16), "cube24": lambda: poisson3d(24),
    "nine24": lambda: ninepoint(24), "nine64": lambda: ninepoint(64),
    "graph1500": lambda: knn_laplacian(1500, seed=1500), "graph6000": lambda: knn_laplacian(6000, seed=6000),
    "arrow3000": arrow,
    "split33": lambda: as_a_file_gives_it("split33"),
}


@functools.lru_cache(maxsize=None)
def system(name):
    """(matrix, structure of its automatic hierarchy at theta = 0.08), built once, never written."""
    M = SYSTEMS[name]()
    return M, structure(M)


def vectors(name):
    """b ~ N(0, 1) seeded by the name's rows, x0 = 0."""
    n = rows_of(system(name)[0])
    return np.random.default_rng(n).standard_normal(n), np.zeros(n)


def upwind33():
    """The nonsymmetric row of the table: the 33 x 33 upwind convection-diffusion stencil of the GCR tests (grid33), b, x0."""
    import gcr_restatement as GR
    A, b, x0 = GR.table_system("grid33")
    return csr_of(A), b, x0


def oneway33():
    """The second nonsymmetric row: oneway33 of tests/poison.py, b ~ N(0, 1) seeded by its rows, x0 = 0."""
    M = as_a_file_gives_it("oneway33")
    n = rows_of(M)
    return M, np.random.default_rng(n).standard_normal(n), np.zeros(n)


# (system, nu, iterations of AMG-PCG in both CPU roundings at tol 1e-6 from x0 = 0, b ~ N(0, 1)); JACOBI: the Jacobi-PCG counts of the
# same restatement. tests/test_amg_host.py re-runs every row in both roundings.
TABLE = [
    ("poisson33", 0, 18), ("poisson33", 1, 12), ("poisson33", 2, 10),
    ("poisson64", 0, 23), ("poisson64", 1, 16), ("poisson64", 2, 13),
    ("poisson127", 0, 29), ("poisson127", 1, 19), ("poisson127", 2, 16),
    ("permuted64", 0, 26), ("permuted64", 1, 16), ("permuted64", 2, 13),
    ("aniso64", 0, 31), ("aniso64", 1, 19), ("aniso64", 2, 16),
    ("cube9", 0, 13), ("cube9", 1, 8), ("cube9", 2, 6),
    ("cube16", 0, 16), ("cube16", 1, 10), ("cube16", 2, 8),
    ("cube24", 0, 19), ("cube24", 1, 12), ("cube24", 2, 10),
    ("nine24", 0, 12), ("nine24", 1, 9), ("nine24", 2, 7),
    ("nine64", 0, 18), ("nine64", 1, 13), ("nine64", 2, 10),
    ("graph1500", 0, 25), ("graph1500", 1, 18), ("graph1500", 2, 15),
    ("graph6000", 0, 29), ("graph6000", 1, 19), ("graph6000", 2, 16),
    ("split33", 1, 12),
]
JACOBI = {"poisson33": 87, "poisson64": 152, "poisson127": 320, "permuted64": 166, "aniso64": 275, "cube9": 31, "cube16": 52,
          "cube24": 74, "nine24": 46, "nine64": 107, "graph1500": 193, "graph6000": 338, "split33": 87}
# the level rows of the automatic hierarchies (theta = 0.08)
LEVEL_ROWS = {"poisson33": [1089, 195, 28], "poisson64": [4096, 704, 88, 17], "poisson127": [16129, 2720, 319, 54],
              "permuted64": [4096, 588, 78, 8], "aniso64": [4096, 1408, 512, 192, 64], "cube9": [729, 96, 14],
              "cube16": [4096, 514, 74, 11], "cube24": [13824, 1685, 215, 31], "nine24": [576, 64], "nine64": [4096, 484, 88, 14],
              "graph1500": [1500, 137, 20], "graph6000": [6000, 523, 75, 11], "split33": [1089, 195, 28]}
# GCR(16) on upwind33 at nu = 1, tol 1e-6: iterations in both CPU roundings
GCR_ROW = ("upwind33", 1, 16, 10)
GCR_ROW_ONEWAY = ("oneway33", 1, 16, 16)  # the same on oneway33 (levels 1089, 198, 30)
