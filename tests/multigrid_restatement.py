"""numpy restatement of the aggregation multigrid preconditioner of csrc/multigrid.hip (include/spmv_amd/api.h):
the hierarchy of 2 x 2 aggregates with every coarse entry summed in the library's order, the per-level intervals and coefficients, the
V-cycle -- bit for bit when it is given each level's own product and a fused multiply-add (the oracle's spmv_stencil5 and axpy), to
rounding with plain numpy --, the preconditioned loop in two roundings, and the table of systems the whole-solve tests use."""
import numpy as np
import scipy.sparse as sp

import chebyshev_restatement as R
from pcg_restatement import diagonal

COARSEST_GRID = 8
COARSEST_DEGREE = 8
FINE_RATIO = 4.0      # smoother interval [lambda_max / 4, lambda_max]
COARSEST_RATIO = 30.0


def grids(n0, max_levels=0):
    """n_0, n_1 = ceil(n_0 / 2), ...: stops at the first grid <= 8, or at max_levels."""
    out = [n0]
    while out[-1] > COARSEST_GRID and (max_levels == 0 or len(out) < max_levels):
        out.append((out[-1] + 1) // 2)
    return out


def sorted_csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def coarsen(A, n):
    """A_c = P^T A P of an n x n 5-point stencil (sorted CSR) on the ceil(n / 2) grid, every coarse entry a sequential sum from 0.0: the
    members of an aggregate in the order (0,0), (0,1), (1,0), (1,1), each member's entries in CSR order, every entry added to the coarse
    entry of the aggregate its column lies in. All coarse rows advance together, one (member, slot) at a time."""
    A = sorted_csr(A)
    nc = (n + 1) // 2
    I, J = np.divmod(np.arange(nc * nc), nc)
    length = np.diff(A.indptr)
    bucket = {k: np.zeros(nc * nc) for k in "nwces"}
    for a in (0, 1):
        for b in (0, 1):
            i, j = 2 * I + a, 2 * J + b
            exists = (i < n) & (j < n)
            fr = np.where(exists, i * n + j, 0)
            for k in range(5):
                live = np.nonzero(exists & (length[fr] > k))[0]
                at = A.indptr[fr[live]] + k
                c = A.indices[at]
                CI, CJ = (c // n) // 2, (c % n) // 2
                v = A.data[at]
                inside = (CI == I[live]) & (CJ == J[live])
                north, south = CI < I[live], CI > I[live]
                west = ~inside & ~north & ~south & (CJ < J[live])
                east = ~inside & ~north & ~south & (CJ > J[live])
                for name, mask in (("c", inside), ("n", north), ("s", south), ("w", west), ("e", east)):
                    rows = live[mask]
                    bucket[name][rows] = bucket[name][rows] + v[mask]
    row = np.arange(nc * nc)
    parts = [(I > 0, row - nc, "n"), (J > 0, row - 1, "w"), (np.ones(nc * nc, bool), row, "c"), (J < nc - 1, row + 1, "e"),
             (I < nc - 1, row + nc, "s")]
    rows = np.concatenate([row[m] for m, _, _ in parts])
    cols = np.concatenate([col[m] for m, col, _ in parts])
    vals = np.concatenate([bucket[name][m] for m, _, name in parts])
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nc * nc))])
    return sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr.astype(np.int32)), shape=(nc * nc, nc * nc))


def prolongation(n):
    """P (n^2 x nc^2), piecewise constant over the 2 x 2 aggregates."""
    nc = (n + 1) // 2
    i, j = np.divmod(np.arange(n * n), n)
    return sp.csr_matrix((np.ones(n * n), ((i * n + j), (i // 2) * nc + j // 2)), shape=(n * n, nc * nc))


class Level:
    def __init__(self, n, A, dinv, lambda_max, coef):
        self.n, self.A, self.dinv, self.lambda_max, self.coef = n, A, dinv, lambda_max, coef


def hierarchy(A, n, nu, max_levels=0, lambda_max=None):
    """The levels of the library's hierarchy. lambda_max: the library's reported bounds (one per level) instead of the restatement's
    own Gershgorin bounds -- the GPU tests hold the bound to 4 ulp and run the rest on the reported one."""
    levels = []
    ns = grids(n, max_levels)
    A = sorted_csr(A)
    for l, nl in enumerate(ns):
        if l > 0:
            A = coarsen(A, ns[l - 1])
        dinv = 1.0 / diagonal(A)
        hi = float(lambda_max[l]) if lambda_max is not None else R.gershgorin(A, dinv)
        last = l == len(ns) - 1
        lo = hi / COARSEST_RATIO if last else hi / FINE_RATIO
        levels.append(Level(nl, A, dinv, hi, R.coefficients(COARSEST_DEGREE if last else nu, lo, hi)))
    return levels


def restrict(t, n):
    """r_c[I, J] = ((t00 + t01) + t10) + t11 over the members that exist."""
    T = t.reshape(n, n)
    h = n // 2
    acc = T[0::2, 0::2].copy()
    acc[:, :h] = acc[:, :h] + T[0::2, 1::2]
    acc[:h, :] = acc[:h, :] + T[1::2, 0::2]
    acc[:h, :h] = acc[:h, :h] + T[1::2, 1::2]
    return acc.ravel()


def prolong(ec, n):
    nc = (n + 1) // 2
    return np.repeat(np.repeat(ec.reshape(nc, nc), 2, axis=0), 2, axis=1)[:n, :n].ravel()


def make_cycle(levels, matvecs=None, fma=None):
    """r -> z = M^-1 r, one V-cycle. matvecs[l]: level l's product (the operator's own bits for the bit-exact form; default A_l @ v);
    fma(a, x, y) = a * x + y rounded once (the oracle's axpy); None: two roundings."""
    if fma is None:
        def fma(a, x, y):
            return a * x + y
    if matvecs is None:
        matvecs = [(lambda v, A=L.A: A @ v) for L in levels]

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
        rc = restrict(fma(-1.0, mv(z), r), L.n)
        ec = cycle(l + 1, rc)
        z = fma(2.0, prolong(ec, L.n), z)
        d, z = update(L, mv, r, d, z, L.coef[0], 0.0)
        for k in range(1, degree + 1):
            d, z = update(L, mv, r, d, z, L.coef[2 * k], L.coef[2 * k - 1])
        return z

    return lambda r: cycle(0, r)


def pcg(A, n, b, x0, nu, tol=1e-6, max_iters=1000, max_levels=0, lambda_max=None):
    """Multigrid-PCG. Returns x, history, iterations, converged."""
    A = sorted_csr(A)
    levels = hierarchy(A, n, nu, max_levels, lambda_max)
    return R._loop(lambda v: A @ v, lambda u, v: float(u @ v), b, x0, make_cycle(levels), tol, max_iters)


def pcg_other_rounding(A, n, b, x0, nu, tol=1e-6, max_iters=1000, max_levels=0, lambda_max=None):
    """pcg() with every sum of the loop and the cycle rounded differently: each level's product through its CSC form, the dot products
    in long double."""
    levels = hierarchy(A, n, nu, max_levels, lambda_max)
    csc = [sp.csc_matrix(L.A) for L in levels]
    matvecs = [(lambda v, T=T: T @ v) for T in csc]
    ld = np.longdouble

    def dot(u, v):
        return float(np.sum(u.astype(ld) * v.astype(ld)))

    return R._loop(matvecs[0], dot, b, x0, make_cycle(levels, matvecs), tol, max_iters)


def conductance_stencil(n, seed):
    """An SPD 5-point stencil with random edge conductances U(0.5, 2), the grid's border edges included (they only add to the diagonal):
    off-diagonals -w, diagonal = the sum of the four incident edges. Bit-symmetric."""
    rng = np.random.default_rng(seed)
    hz = rng.uniform(0.5, 2.0, (n, n + 1))  # hz[i, j]: the edge west of (i, j); hz[i, n]: the border edge east of (i, n-1)
    vt = rng.uniform(0.5, 2.0, (n + 1, n))
    diag = ((hz[:, :-1] + hz[:, 1:]) + vt[:-1, :]) + vt[1:, :]
    idx = np.arange(n * n).reshape(n, n)
    rows = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    cols = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    vals = [diag.ravel(), -hz[:, 1:-1].ravel(), -hz[:, 1:-1].ravel(), -vt[1:-1, :].ravel(), -vt[1:-1, :].ravel()]
    return sorted_csr(sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n)))


def table_system(name):
    """A, b, x0 of chebyshev_restatement.table_system, and the grid n."""
    A, b, x0 = R.table_system(name)
    return A, b, x0, int(round(np.sqrt(A.shape[0])))


# (system, nu, tol, iterations the CPU restatement takes in both roundings), all on the automatic hierarchy. The two roundings' histories
# agree to 1e-13 or better on every row (tests/test_multigrid_host.py re-runs the comparison and asserts 1e-12). Left out because they do not:
# poisson513 -- odd at every level, so every level has one-point aggregates on two edges, which the factor 2 over-corrects; M^-1 A
# then has a few large outlying eigenvalues (a 65 grid: [0.81, 4.7] against [0.79, 1.85] at 64), CG's Ritz values find them within a
# few iterations and what follows depends on the rounding (counts 18 / 30 / 14 at nu = 1 / 0 / 2 in both roundings, histories 7.5e-7 /
# 2.7e-1 / 4.6e-9 apart) -- and the tol = 1e-10 rows of poisson255 / poisson640 (2.8e-12 / 3.0e-10 apart). negated65 keeps a hierarchy
# that is odd at every level (65, 33, 17, 9, 5) in the table.
TABLE = [
    ("poisson127", 1, 1e-6, 10), ("poisson127", 0, 1e-6, 17), ("poisson127", 2, 1e-6, 8), ("poisson127", 1, 1e-10, 17),
    ("poisson255", 1, 1e-6, 12), ("poisson255", 0, 1e-6, 20), ("poisson255", 2, 1e-6, 9),
    ("poisson640", 1, 1e-6, 12), ("poisson640", 2, 1e-6, 9),
    ("plain127", 1, 1e-6, 6), ("plain601", 1, 1e-6, 6), ("plain601", 2, 1e-6, 5),
    ("scaled127", 1, 1e-6, 6), ("scaled127", 1, 1e-10, 10), ("scaled601", 1, 1e-6, 6), ("scaled601", 0, 1e-6, 10),
    ("negated65", 1, 1e-6, 5), ("negated65", 0, 1e-6, 9), ("negated65", 2, 1e-6, 4), ("negated65", 1, 1e-10, 9),
]
