"""numpy restatement of the restarted GCR loop of spmv_amd_gcr_solve_device (csrc/gcr.hip; api.h states the
algebra) on the nonsymmetric systems of bicgstab_restatement. A kind is "none", "jacobi", "chebyshev<K>" or "multigrid<NU>".

Three forms of one loop: gcr() in plain numpy (products in row order, numpy dots, a * b + c rounded twice, the applications of
chebyshev_restatement.make_apply / multigrid_restatement.make_cycle in the same arithmetic), gcr_other_rounding() (products through the
CSC forms -- the levels' included --, long-double dots) -- what the two disagree by on an input is what a comparison against either
can mean on that input -- and gcr_exact(): every dot product as the kernels sum it (reduction_restatement.stream_partials +
reduce_pcg), every update through the oracle's fma, the product and the application handed in by the caller in the operator's own
bits (exact_apply builds the application from the oracle's products; the GPU tests may hand in the library's own
spmv_amd_precond_apply_device, which the preconditioners' tests hold bit for bit). The device must equal the last bit for bit."""
import functools

import numpy as np
import scipy.sparse as sp

import chebyshev_restatement as CH
import multigrid3d_restatement as MG3
import multigrid_restatement as MG
from bicgstab_restatement import (SYSTEMS, _below, _unusable, convdiff5, convdiff7, diagonal, entries_of, hist_err,  # noqa: F401
                                  table_system, true_residual_norm)

MAX_RESTART = 32
DEFAULT_RESTART = 16


def _loop(matvec, dot, b, x0, apply, restart, tol, max_iters, fma=lambda a, b, c: a * b + c):
    """The algebra of api.h, step for step. Returns x, history, iterations, converged, and how it ended: "converged", "gamma", "rho"
    or "max_iters"."""
    m = DEFAULT_RESTART if restart == 0 else restart
    assert 1 <= m <= MAX_RESTART
    x = np.array(x0, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    r = b - matvec(x)  # fma(1.0, b, -1.0 * Ax): the difference rounded once
    b_norm = float(np.sqrt(dot(r, r)))
    hist = [b_norm]
    Q, Z, gammas = [], [], []
    it, converged, end = 0, False, "max_iters"
    for k in range(max_iters):
        j = k % m
        if j == 0:
            Q, Z, gammas = [], [], []
        z = apply(r)
        q = matvec(z)
        with np.errstate(divide="ignore", invalid="ignore"):
            betas = [np.float64(dot(Q[i], q)) / np.float64(gammas[i]) for i in range(j)]  # all from the q of the product
        for i in range(j):
            q = fma(-float(betas[i]), Q[i], q)
            z = fma(-float(betas[i]), Z[i], z)
        gamma, rho = dot(q, q), dot(r, q)
        it += 1
        if _unusable(gamma) or _unusable(rho):
            hist.append(hist[-1])
            end = "gamma" if _unusable(gamma) else "rho"
            break
        alpha = rho / gamma
        x = fma(alpha, z, x)
        r = fma(-alpha, q, r)
        res = float(np.sqrt(dot(r, r)))
        hist.append(res)
        if _below(res, b_norm, tol):
            converged, end = True, "converged"
            break
        Q.append(q), Z.append(z), gammas.append(gamma)
    return x, np.array(hist), it, converged, end


def parse_kind(kind):
    """"chebyshev2" -> ("chebyshev", 2); "none" -> ("none", None)."""
    for name in ("chebyshev", "multigrid"):
        if kind.startswith(name):
            return name, int(kind[len(name):])
    assert kind in ("none", "jacobi"), kind
    return kind, None


def grid_of(A, dim):
    return int(round(A.shape[0] ** (1.0 / dim)))


def make_apply(A, dim, kind, csc=False, lambda_max=None):
    """r -> z = M^-1 r in numpy arithmetic. csc: every product (the levels' too) through the CSC form. lambda_max: the library's
    reported bound(s) instead of the restatement's own Gershgorin bounds."""
    name, k = parse_kind(kind)
    if name == "none":
        return lambda r: r
    dinv = 1.0 / diagonal(A)
    if name == "jacobi":
        return lambda r: dinv * r
    form = sp.csc_matrix if csc else sp.csr_matrix
    if name == "chebyshev":
        T = form(A)
        lo, hi = CH.interval(A, dinv, 0.0, 0.0 if lambda_max is None else float(lambda_max))
        return CH.make_apply(lambda v: T @ v, dinv, CH.coefficients(k, lo, hi))
    M = MG if dim == 2 else MG3
    levels = M.hierarchy(A, grid_of(A, dim), k, lambda_max=lambda_max)
    forms = [form(L.A) for L in levels]
    return M.make_cycle(levels, [(lambda v, T=T: T @ v) for T in forms])


def exact_apply(O, A, dim, kind, lambda_max=None):
    """r -> z = M^-1 r bit for bit as the library applies it on stencil5-csr (dim 2: the oracle's stencil product on every level) or
    stencil7-csr (dim 3: the CSR loop), every update an fma. lambda_max as in make_apply."""
    name, k = parse_kind(kind)
    if name == "none":
        return lambda r: r
    dinv = 1.0 / diagonal(A)
    if name == "jacobi":
        return lambda r: dinv * r

    def product(M_, n):
        M_ = MG.sorted_csr(M_)
        rp, ci, va = M_.indptr.astype(np.int32), M_.indices.astype(np.int32), np.ascontiguousarray(M_.data)
        return (lambda v: O.spmv_stencil5(rp, ci, va, v, n)) if dim == 2 else (lambda v: O.spmv_csr(rp, ci, va, v))

    n = grid_of(A, dim)
    if name == "chebyshev":
        lo, hi = CH.interval(A, dinv, 0.0, 0.0 if lambda_max is None else float(lambda_max))
        return CH.make_apply(product(A, n), dinv, CH.coefficients(k, lo, hi), fma=O.axpy)
    M = MG if dim == 2 else MG3
    levels = M.hierarchy(A, n, k, lambda_max=lambda_max)
    return M.make_cycle(levels, [product(L.A, L.n) for L in levels], fma=O.axpy)


def gcr(A, b, x0, apply, restart=0, tol=1e-6, max_iters=1000):
    """Returns x, history (the recorded norms, k = 0..iterations), iterations, converged, end."""
    A = sp.csr_matrix(A)
    return _loop(lambda u: A @ u, lambda u, v: float(u @ v), b, x0, apply, restart, tol, max_iters)


def gcr_other_rounding(A, b, x0, apply, restart=0, tol=1e-6, max_iters=1000):
    """gcr() with every sum rounded differently: the product through the CSC form of A and the dot products in long double, as
    pcg_restatement.pcg_other_rounding does; hand in make_apply(..., csc=True) for the application."""
    T = sp.csc_matrix(A)
    ld = np.longdouble

    def dot(u, v):
        return float(np.sum(u.astype(ld) * v.astype(ld)))

    return _loop(lambda u: T @ u, dot, b, x0, apply, restart, tol, max_iters)


def exact_dot(u, v):
    """One dot product as the kernels sum it: the streaming partials, then pcg_reduce_kernel's geometry."""
    import reduction_restatement as R

    return R.reduce_pcg(R.stream_partials(u, v), R.stream_count(len(u)), 1)[0]


def gcr_exact(matvec, b, x0, apply, restart=0, tol=1e-6, max_iters=1000):
    """The device's bits: matvec is the operator's own product (oracle.spmv_stencil5 for stencil5-csr, oracle.spmv_csr for the
    sequential CSR operators and stencil7-csr), apply the application in the library's bits, every dot product the streaming partials
    summed by reduce_pcg, every update the oracle's fma."""
    from oracle import oracle as O

    def fma(a, u, c):
        return O.fma(np.full(len(u), a), u, c)

    return _loop(matvec, exact_dot, b, x0, apply, restart, tol, max_iters, fma)


def dimension_of(name):
    return SYSTEMS[name][0]


@functools.lru_cache(maxsize=None)
def two_roundings(name, kind, restart, tol):
    """One table row in plain numpy and in the other rounding."""
    A, b, x0 = table_system(name)
    dim = dimension_of(name)
    return (gcr(A, b, x0, make_apply(A, dim, kind), restart, tol),
            gcr_other_rounding(A, b, x0, make_apply(A, dim, kind, csc=True), restart, tol))


# (system, kind, restart, tol, iterations both CPU roundings take, their largest relative history disagreement: stored as twice what
# tests/test_gcr_host.py measures, which it prints, and never below 1e-14: a disagreement of a few ulp of one norm is the summation
# order of one dot product, no property of the row). Every row converges. The "jacobi" counts equal the "none" counts on the
# constant-diagonal systems, so those systems carry "none" only; the row-scaled system carries "jacobi" ("none" there is no property
# of the input). The stored figure is ONE sample of what re-rounding does to the row: a third rounding of the same algebra --
# gcr_exact, and the device, which equals it bit for bit -- is held against plain numpy to third_rounding_bound(stored).
TABLE = [
    ("grid33", "none", 4, 1e-06, 49, 1e-14),
    ("grid33", "none", 4, 1e-10, 73, 2e-14),
    ("grid33", "none", 16, 1e-06, 48, 1e-14),
    ("grid33", "none", 16, 1e-10, 75, 6e-14),
    ("grid33", "multigrid1", 4, 1e-06, 10, 3e-13),
    ("grid33", "multigrid1", 4, 1e-10, 17, 3e-13),
    ("grid33", "multigrid1", 16, 1e-06, 10, 1e-14),
    ("grid33", "multigrid1", 16, 1e-10, 16, 4e-12),
    ("grid65", "none", 4, 1e-06, 61, 1e-14),
    ("grid65", "none", 4, 1e-10, 103, 1e-14),
    ("grid65", "none", 16, 1e-06, 61, 1e-14),
    ("grid65", "none", 16, 1e-10, 99, 4e-14),
    ("grid65", "multigrid1", 4, 1e-06, 11, 3e-14),
    ("grid65", "multigrid1", 4, 1e-10, 19, 8e-14),
    ("grid65", "multigrid1", 16, 1e-06, 11, 1e-14),
    ("grid65", "multigrid1", 16, 1e-10, 18, 8e-09),
    ("grid127", "none", 4, 1e-06, 63, 1e-14),
    ("grid127", "none", 4, 1e-10, 118, 1e-14),
    ("grid127", "none", 16, 1e-06, 63, 1e-14),
    ("grid127", "none", 16, 1e-10, 118, 1e-14),
    ("grid127", "multigrid1", 4, 1e-06, 12, 1e-14),
    ("grid127", "multigrid1", 4, 1e-10, 21, 2e-14),
    ("grid127", "multigrid1", 16, 1e-06, 12, 1e-14),
    ("grid127", "multigrid1", 16, 1e-10, 20, 5e-09),
    ("rows127", "jacobi", 4, 1e-06, 61, 1e-14),
    ("rows127", "jacobi", 4, 1e-10, 116, 1e-14),
    ("rows127", "jacobi", 16, 1e-06, 61, 1e-14),
    ("rows127", "jacobi", 16, 1e-10, 115, 1e-14),
    ("rows127", "multigrid1", 4, 1e-06, 33, 1e-14),
    ("rows127", "multigrid1", 4, 1e-10, 59, 1e-14),
    ("rows127", "multigrid1", 16, 1e-06, 31, 6e-14),
    ("rows127", "multigrid1", 16, 1e-10, 54, 3e-13),
    ("cube16", "none", 4, 1e-06, 39, 1e-14),
    ("cube16", "none", 4, 1e-10, 62, 2e-14),
    ("cube16", "none", 16, 1e-06, 37, 4e-13),
    ("cube16", "none", 16, 1e-10, 61, 2e-12),
    ("cube16", "chebyshev2", 4, 1e-06, 27, 1e-14),
    ("cube16", "chebyshev2", 4, 1e-10, 36, 7e-14),
    ("cube16", "multigrid1", 4, 1e-06, 7, 1e-14),
    ("cube16", "multigrid1", 4, 1e-10, 13, 2e-13),
    ("cube16", "multigrid1", 16, 1e-06, 7, 1e-14),
    ("cube16", "multigrid1", 16, 1e-10, 13, 2e-14),
]

# What apps/cg_solver --solver=gcr:4 --precond=multigrid solves on a Matrix Market file: convdiff5 on the 33 grid, b = 1, x0 = 0,
# tol 1e-6. (grid, restart, kind, iterations in both CPU roundings and in the exact form.)
APP_CASE = (33, 4, "multigrid1", 11)


def third_rounding_bound(stored):
    """What another rounding of a table row (gcr_exact, the device) may differ by from gcr(): history and x, relative -- the rule of
    bicgstab_restatement.third_rounding_bound."""
    return max(1e-10, 10.0 * stored)
