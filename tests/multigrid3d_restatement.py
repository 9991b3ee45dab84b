"""numpy restatement of the aggregation multigrid preconditioner on the 3-D operator (csrc/multigrid3d.hip and the cycle of
csrc/multigrid.hip, DESIGN.md section 17, include/spmv_amd/api.h): the hierarchy of 2 x 2 x 2 aggregates with every coarse entry summed in
the library's order, restriction and prolongation, the V-cycle -- multigrid_restatement.make_cycle itself, given this file's restriction
and prolongation; bit for bit when it is given each level's own product and a fused multiply-add (the oracle's spmv_csr and axpy) --,
the preconditioned loop in two roundings, a random-conductance generator, and the table of systems the whole-solve tests use.
Point (k, i, j) of an n^3 grid is row k n^2 + i n + j; a complete row is [D,N,W,C,E,S,U] = columns -n^2, -n, -1, 0, +1, +n, +n^2."""
import types

import numpy as np
import scipy.sparse as sp

import chebyshev_restatement as R
import multigrid_restatement as MG
import stencil7 as S7
from pcg_restatement import diagonal

grids = MG.grids          # n_{l+1} = ceil(n_l / 2), the first grid <= 8 or max_levels: the same rule in 3-D
sorted_csr = MG.sorted_csr
MEMBERS = [(c, a, b) for c in (0, 1) for a in (0, 1) for b in (0, 1)]  # the order of every sum over an aggregate


def coarsen(A, n):
    """A_c = P^T A P of an n^3 7-point stencil (sorted CSR) on the ceil(n / 2)^3 grid, every coarse entry a sequential sum from 0.0:
    the members of an aggregate in the order MEMBERS, each member's entries in CSR order, every entry added to the coarse entry of the
    aggregate its column lies in. All coarse rows advance together, one (member, slot) at a time."""
    A = sorted_csr(A)
    nc = (n + 1) // 2
    row = np.arange(nc ** 3)
    K, rest = np.divmod(row, nc * nc)
    I, J = np.divmod(rest, nc)
    length = np.diff(A.indptr)
    bucket = {k: np.zeros(nc ** 3) for k in "dnwcesu"}
    for c, a, b in MEMBERS:
        k, i, j = 2 * K + c, 2 * I + a, 2 * J + b
        exists = (k < n) & (i < n) & (j < n)
        fr = np.where(exists, (k * n + i) * n + j, 0)
        for slot in range(7):
            live = np.nonzero(exists & (length[fr] > slot))[0]
            at = A.indptr[fr[live]] + slot
            col = A.indices[at].astype(np.int64)
            ck, crest = np.divmod(col, n * n)
            ci, cj = np.divmod(crest, n)
            CK, CI, CJ = ck // 2, ci // 2, cj // 2
            v = A.data[at]
            Kl, Il, Jl = K[live], I[live], J[live]
            masks = {"d": CK < Kl, "u": CK > Kl}
            same_k = CK == Kl
            masks["n"], masks["s"] = same_k & (CI < Il), same_k & (CI > Il)
            same_ki = same_k & (CI == Il)
            masks["w"], masks["e"], masks["c"] = same_ki & (CJ < Jl), same_ki & (CJ > Jl), same_ki & (CJ == Jl)
            for name, mask in masks.items():
                rows = live[mask]
                bucket[name][rows] = bucket[name][rows] + v[mask]
    parts = [(K > 0, row - nc * nc, "d"), (I > 0, row - nc, "n"), (J > 0, row - 1, "w"), (np.ones(nc ** 3, bool), row, "c"),
             (J < nc - 1, row + 1, "e"), (I < nc - 1, row + nc, "s"), (K < nc - 1, row + nc * nc, "u")]
    rows = np.concatenate([row[m] for m, _, _ in parts])
    cols = np.concatenate([col[m] for m, col, _ in parts])
    vals = np.concatenate([bucket[name][m] for m, _, name in parts])
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nc ** 3))])
    return sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr.astype(np.int32)), shape=(nc ** 3, nc ** 3))


def prolongation(n):
    """P (n^3 x nc^3), piecewise constant over the 2 x 2 x 2 aggregates."""
    nc = (n + 1) // 2
    r = np.arange(n ** 3)
    k, rest = np.divmod(r, n * n)
    i, j = np.divmod(rest, n)
    return sp.csr_matrix((np.ones(n ** 3), (r, ((k // 2) * nc + i // 2) * nc + j // 2)), shape=(n ** 3, nc ** 3))


def restrict(t, n):
    """r_c[K, I, J] = (((((((t000 + t001) + t010) + t011) + t100) + t101) + t110) + t111) over the members that exist."""
    T = t.reshape(n, n, n)
    h = n // 2
    acc = T[0::2, 0::2, 0::2].copy()  # t000 exists in every aggregate
    for c, a, b in MEMBERS[1:]:
        part = T[c::2, a::2, b::2]
        sk, si, sj = (slice(0, h) if c else slice(None)), (slice(0, h) if a else slice(None)), (slice(0, h) if b else slice(None))
        acc[sk, si, sj] = acc[sk, si, sj] + part
    return acc.ravel()


def prolong(ec, n):
    nc = (n + 1) // 2
    E = ec.reshape(nc, nc, nc)
    return np.repeat(np.repeat(np.repeat(E, 2, axis=0), 2, axis=1), 2, axis=2)[:n, :n, :n].ravel()


def hierarchy(A, n, nu, max_levels=0, lambda_max=None):
    """The levels of the library's hierarchy (multigrid_restatement.Level). lambda_max: the library's reported bounds (one per level)
    instead of the restatement's own Gershgorin bounds."""
    levels = []
    ns = grids(n, max_levels)
    A = sorted_csr(A)
    for l, nl in enumerate(ns):
        if l > 0:
            A = coarsen(A, ns[l - 1])
        dinv = 1.0 / diagonal(A)
        hi = float(lambda_max[l]) if lambda_max is not None else R.gershgorin(A, dinv)
        last = l == len(ns) - 1
        lo = hi / MG.COARSEST_RATIO if last else hi / MG.FINE_RATIO
        levels.append(MG.Level(nl, A, dinv, hi, R.coefficients(MG.COARSEST_DEGREE if last else nu, lo, hi)))
    return levels


# The cycle is multigrid_restatement.make_cycle, statement for statement: the same function body run with this file's restrict and
# prolong in place of the 2-D ones it names (section 17: "the cycle is section 15's with two changes").
make_cycle = types.FunctionType(MG.make_cycle.__code__, {**vars(MG), "restrict": restrict, "prolong": prolong}, "make_cycle",
                                MG.make_cycle.__defaults__)


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


def matrix_of(e, n):
    return sorted_csr(sp.csr_matrix((e["value"], (e["row"], e["col"])), shape=(n ** 3, n ** 3)))


def poisson(n):
    """centre 6, neighbours -1 (Dirichlet boundary)"""
    return matrix_of(S7.coo(n, center=6.0, off=-1.0), n)


def conductance_stencil(n, seed):
    """An SPD 7-point stencil with random edge conductances U(0.5, 2), the cube's border edges included (they only add to the
    diagonal): off-diagonals -w, diagonal = the sum of the six incident edges, x edges then y then z. Bit-symmetric."""
    rng = np.random.default_rng(seed)
    ex = rng.uniform(0.5, 2.0, (n, n, n + 1))  # ex[k, i, j]: the edge west of (k, i, j)
    ey = rng.uniform(0.5, 2.0, (n, n + 1, n))
    ez = rng.uniform(0.5, 2.0, (n + 1, n, n))
    diag = ((((ex[:, :, :-1] + ex[:, :, 1:]) + ey[:, :-1, :]) + ey[:, 1:, :]) + ez[:-1, :, :]) + ez[1:, :, :]
    idx = np.arange(n ** 3).reshape(n, n, n)
    rows = [idx.ravel(), idx[:, :, 1:].ravel(), idx[:, :, :-1].ravel(), idx[:, 1:, :].ravel(), idx[:, :-1, :].ravel(), idx[1:].ravel(),
            idx[:-1].ravel()]
    cols = [idx.ravel(), idx[:, :, :-1].ravel(), idx[:, :, 1:].ravel(), idx[:, :-1, :].ravel(), idx[:, 1:, :].ravel(), idx[:-1].ravel(),
            idx[1:].ravel()]
    wx, wy, wz = -ex[:, :, 1:-1].ravel(), -ey[:, 1:-1, :].ravel(), -ez[1:-1].ravel()
    vals = [diag.ravel(), wx, wx, wy, wy, wz, wz]
    return sorted_csr(sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3)))


def table_system(name):
    """A, b, x0 and the grid n. "poisson<n>": centre 6, neighbours -1; "conductance<n>": conductance_stencil(n, seed n);
    "generator<n>": the operator's synthetic matrix (centre 7, neighbours -1). rng = default_rng(3000 + n), b then x0 ~ N(0, 1)."""
    for kind in ("poisson", "conductance", "generator"):
        if name.startswith(kind):
            n = int(name[len(kind):])
            break
    else:
        raise KeyError(name)
    A = poisson(n) if kind == "poisson" else conductance_stencil(n, n) if kind == "conductance" else matrix_of(S7.coo(n), n)
    rng = np.random.default_rng(3000 + n)
    b = rng.standard_normal(n ** 3)
    x0 = rng.standard_normal(n ** 3)
    return A, b, x0, n


MARGIN = 0.15  # a table row keeps the residuals of its last two iterations this far (relative) from tol * ||r0||


def row_is_clear(h, tol):
    """The table's third condition: the converging residual and the one before it are at least MARGIN away from tol * ||r0||, so the
    count does not hang on one rounding."""
    bound = tol * h[0]
    return h[-1] <= (1.0 - MARGIN) * bound and h[-2] >= (1.0 + MARGIN) * bound


# (system, nu, tol, iterations the CPU restatement takes in both roundings), all on the automatic hierarchy. A row is here only if both
# roundings give the same count, their histories agree to 1e-12 (tests/test_multigrid3d_host.py re-runs both and asserts it) and
# row_is_clear() holds in both. Run and left out by that rule: poisson32 nu 1 tol 1e-6 (7 iterations, the last residual 0.997 of the
# bound), poisson40 nu 1 (0.928), poisson33 nu 1 (the one before the last 1.10), poisson64 nu 2 (1.08), conductance32 (1.04); and by
# the histories: poisson33 at nu 0 (4.8e-10 apart) and at nu 1 with tol 1e-10 (7.2e-9) -- a grid that is odd at every level has
# one-point aggregates on three faces, which the factor 2 over-corrects, as in 2-D (multigrid_restatement.TABLE has the account).
# poisson17, poisson33 nu 2 and poisson65 keep hierarchies that are odd at every level in the table.
TABLE = [
    ("poisson16", 0, 1e-6, 11), ("poisson16", 1, 1e-6, 6), ("poisson16", 2, 1e-6, 5), ("poisson17", 1, 1e-6, 8),
    ("poisson20", 1, 1e-6, 7), ("poisson32", 0, 1e-6, 15), ("poisson32", 2, 1e-6, 6), ("poisson32", 1, 1e-10, 13),
    ("poisson33", 2, 1e-6, 8), ("conductance48", 1, 1e-6, 10), ("generator48", 1, 1e-6, 7),
    ("poisson64", 1, 1e-6, 9), ("poisson65", 1, 1e-6, 12),
]
