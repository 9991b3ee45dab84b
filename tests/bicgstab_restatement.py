"""numpy restatement of the BiCGSTAB loop of spmv_amd_bicgstab_solve_device (csrc/bicgstab.hip; api.h states
the algebra) and the nonsymmetric matrices its tests use. dinv = None means kind "none" (a hat is the vector itself).

Three forms of one loop: bicgstab() in plain numpy (products in row order, numpy dots, a * b + c rounded twice), bicgstab_other_rounding()
(products through the CSC form, long-double dots) -- what the two disagree by on an input is what a comparison against either can
mean on that input -- and bicgstab_exact(): every dot product as the kernels sum it (reduction_restatement.stream_partials +
reduce_pcg), every update through the oracle's fma, the product handed in by the caller in the operator's own bits. The device must
equal the last bit for bit."""
import functools

import numpy as np
import scipy.sparse as sp

from pcg_restatement import diagonal, entries_of, hist_err, true_residual_norm  # noqa: F401  (re-exported to the tests)


def convdiff5(n, px=2.0, py=0.5, shift=0.5, decades=0.0, seed=0):
    """5-point upwind convection-diffusion on an n x n grid (scipy CSR): centre 4 + px + py + shift, W = -1 - px, N = -1 - py,
    E = S = -1. Nonsymmetric: |A - A^T| reaches px. decades > 0: diag(10^U(0, decades)) A, a row scaling drawn from `seed`."""
    t = sp.diags([np.full(n - 1, -1.0 - px), np.full(n, 4.0 + px + py + shift), np.full(n - 1, -1.0)], [-1, 0, 1])
    eye = sp.identity(n)
    A = sp.kron(eye, t) + sp.kron(sp.diags([np.full(n - 1, -1.0 - py), np.full(n - 1, -1.0)], [-1, 1]), eye)
    return _row_scaled(sp.csr_matrix(A), decades, seed)


def convdiff7(n, px=2.0, py=0.5, pz=1.0, shift=0.5, decades=0.0, seed=0):
    """The 3-D twin on an n x n x n grid: centre 6 + px + py + pz + shift, W = -1 - px, N = -1 - py, D = -1 - pz, E = S = U = -1."""
    t = sp.diags([np.full(n - 1, -1.0 - px), np.full(n, 6.0 + px + py + pz + shift), np.full(n - 1, -1.0)], [-1, 0, 1])
    eye = sp.identity(n)
    ny = sp.diags([np.full(n - 1, -1.0 - py), np.full(n - 1, -1.0)], [-1, 1])
    nz = sp.diags([np.full(n - 1, -1.0 - pz), np.full(n - 1, -1.0)], [-1, 1])
    A = sp.kron(eye, sp.kron(eye, t)) + sp.kron(eye, sp.kron(ny, eye)) + sp.kron(nz, sp.kron(eye, eye))
    return _row_scaled(sp.csr_matrix(A), decades, seed)


def _row_scaled(A, decades, seed):
    if decades == 0.0:
        return A
    s = 10.0 ** np.random.default_rng(seed).uniform(0.0, decades, A.shape[0])
    return sp.csr_matrix(sp.diags(s) @ A)


def _unusable(v):
    return v == 0.0 or not np.isfinite(v)


def _below(norm, b_norm, tol):
    """The strict stopping test, as IEEE division makes it (a zero ||r0|| gives NaN or inf: not below)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float64(norm) / np.float64(b_norm) < tol)


def _loop(matvec, dot, b, x0, dinv, tol, max_iters, fma=lambda a, b, c: a * b + c):
    """The algebra of api.h, step for step. Returns x, history, iterations, converged, and how it ended: "half", "whole", "sigma",
    "omega", "rho" or "max_iters"."""
    hat = (lambda u: u) if dinv is None else (lambda u: dinv * u)
    x = np.array(x0, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    r = b - matvec(x)  # fma(1.0, b, -1.0 * Ax): the difference rounded once
    rhat0 = r.copy()
    p = r.copy()
    ph = hat(p)
    rho = dot(r, r)
    b_norm = float(np.sqrt(rho))
    hist = [b_norm]
    it, converged, end = 0, False, "max_iters"
    for _ in range(max_iters):
        v = matvec(ph)
        sigma = dot(rhat0, v)
        it += 1
        if _unusable(sigma):
            hist.append(hist[-1])
            end = "sigma"
            break
        alpha = rho / sigma
        s = fma(-alpha, v, r)
        sh = hat(s)
        s_norm = float(np.sqrt(dot(s, s)))
        if _below(s_norm, b_norm, tol):
            x = fma(alpha, ph, x)
            hist.append(s_norm)
            converged, end = True, "half"
            break
        t = matvec(sh)
        ts, tt = dot(t, s), dot(t, t)
        if _unusable(tt) or _unusable(ts):
            x = fma(alpha, ph, x)
            r = s
            hist.append(s_norm)
            end = "omega"
            break
        omega = ts / tt
        x = fma(omega, sh, fma(alpha, ph, x))
        r = fma(-omega, t, s)
        res = float(np.sqrt(dot(r, r)))
        hist.append(res)
        if _below(res, b_norm, tol):
            converged, end = True, "whole"
            break
        rho_new = dot(rhat0, r)
        if _unusable(rho_new):
            end = "rho"
            break
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = fma(beta, fma(-omega, v, p), r)
        ph = hat(p)
    return x, np.array(hist), it, converged, end


def bicgstab(A, b, x0, dinv, tol=1e-6, max_iters=1000):
    """Returns x, history (the recorded norms, k = 0..iterations), iterations, converged, end."""
    return _loop(lambda u: A @ u, lambda u, v: float(u @ v), b, x0, dinv, tol, max_iters)


def bicgstab_other_rounding(A, b, x0, dinv, tol=1e-6, max_iters=1000):
    """bicgstab() with every sum rounded differently: the product through the CSC form of A (each y_i accumulated in column order)
    and the dot products in long double, as pcg_restatement.pcg_other_rounding does."""
    T = sp.csc_matrix(A)
    ld = np.longdouble

    def dot(u, v):
        return float(np.sum(u.astype(ld) * v.astype(ld)))

    return _loop(lambda u: T @ u, dot, b, x0, dinv, tol, max_iters)


def bicgstab_exact(matvec, b, x0, dinv, tol=1e-6, max_iters=1000):
    """The device's bits: matvec is the operator's own product (oracle.spmv_stencil5 for stencil5-csr, oracle.spmv_csr for the
    sequential CSR operators and stencil7-csr), every dot product the streaming partials summed by reduce_pcg, every update the
    oracle's fma."""
    import reduction_restatement as R
    from oracle import oracle as O

    def dot(u, v):
        return R.reduce_pcg(R.stream_partials(u, v), R.stream_count(len(u)), 1)[0]

    def fma(a, u, c):
        return O.fma(np.full(len(u), a), u, c)

    return _loop(matvec, dot, b, x0, dinv, tol, max_iters, fma)


# ---------------------------------------------------------------- the systems of the whole-solve tests
# name -> (dimension, grid, decades of row scaling, seed of the scaling, b and x0). px, py, (pz,) shift = 2, 0.5, (1,) 0.5.
SYSTEMS = {"grid33": (2, 33, 0.0, 33), "grid65": (2, 65, 0.0, 65), "grid127": (2, 127, 0.0, 127), "grid601": (2, 601, 0.0, 601),
           "rows127": (2, 127, 2.0, 11), "rows600": (2, 600, 1.0, 13), "cube16": (3, 16, 0.0, 16)}


@functools.lru_cache(maxsize=None)
def table_system(name):
    """Returns A, b, x0 of one system: rng = default_rng(seed), b then x0 = rng.standard_normal(rows)."""
    dim, n, decades, seed = SYSTEMS[name]
    A = convdiff5(n, decades=decades, seed=seed) if dim == 2 else convdiff7(n, decades=decades, seed=seed)
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(A.shape[0])
    x0 = rng.standard_normal(A.shape[0])
    return A, b, x0


def dinv_of(A, kind):
    return 1.0 / diagonal(A) if kind == "jacobi" else None


# (system, kind, tol, iterations both CPU roundings take, how both end, their largest relative history disagreement: stored as twice
# what tests/test_bicgstab_host.py measures, which it prints). Row-scaled systems under kind "none" are no property of the input
# (the roundings take different iteration counts) and stay out, as does anything the roundings drift apart on.
# The stored figure is ONE sample of what re-rounding does to the row: a third rounding of the same algebra -- bicgstab_exact, and the
# device, which equals it bit for bit -- is held against plain numpy to third_rounding_bound(stored) = max(1e-10, 10 x stored).
TABLE = [
    ("grid33", "none", 1e-06, 30, "whole", 6e-11),
    ("grid33", "none", 1e-10, 41, "half", 5e-10),
    ("grid33", "jacobi", 1e-06, 30, "whole", 7e-11),
    ("grid33", "jacobi", 1e-10, 41, "half", 5e-10),
    ("grid65", "none", 1e-06, 34, "half", 3e-10),
    ("grid65", "none", 1e-10, 57, "whole", 6e-9),
    ("grid65", "jacobi", 1e-06, 34, "half", 4e-10),
    ("grid65", "jacobi", 1e-10, 57, "whole", 6e-9),
    ("grid127", "none", 1e-06, 34, "whole", 4e-11),
    ("grid127", "none", 1e-10, 61, "half", 4e-11),
    ("grid127", "jacobi", 1e-06, 34, "whole", 2e-10),
    ("grid127", "jacobi", 1e-10, 61, "half", 2e-10),
    ("grid601", "none", 1e-06, 37, "whole", 9e-11),
    ("grid601", "none", 1e-10, 64, "half", 6e-8),
    ("grid601", "jacobi", 1e-06, 37, "whole", 3e-11),
    ("grid601", "jacobi", 1e-10, 64, "half", 5e-8),
    ("rows127", "jacobi", 1e-06, 37, "half", 3e-9),
    ("rows127", "jacobi", 1e-10, 63, "half", 2e-8),
    ("rows600", "jacobi", 1e-06, 35, "whole", 2e-10),
    ("rows600", "jacobi", 1e-10, 63, "whole", 2e-8),
    ("cube16", "none", 1e-06, 24, "whole", 7e-11),
    ("cube16", "none", 1e-10, 35, "half", 2e-7),
    ("cube16", "jacobi", 1e-06, 24, "whole", 6e-12),
    ("cube16", "jacobi", 1e-10, 35, "half", 8e-8),
]

# What apps/cg_solver solves on a Matrix Market file: b = 1, x0 = 0, tol 1e-6. (grid of convdiff5, iterations both kinds take in
# both CPU roundings and in the exact form on either product; the converging ratio is 0.46, the one before 1.49.)
APP_CASE = (33, 37)


def third_rounding_bound(stored):
    """What another rounding of a table row (bicgstab_exact, the device) may differ by from bicgstab(): history and x, relative."""
    return max(1e-10, 10.0 * stored)
