"""numpy restatement of the Chebyshev polynomial preconditioner of csrc/precond.hip: the coefficient recurrence
in Python floats, the symmetric Gershgorin bound, the application z = M^-1 r -- bit for bit when it is given the operator's own
product and a fused multiply-add (the oracle's spmv_* and axpy), to rounding with plain numpy --, the preconditioned loop of
pcg_restatement._loop with a preconditioner callable, and the table of systems the whole-solve tests use."""
import numpy as np
import scipy.sparse as sp

from pcg_restatement import diagonal, stencil5, table_system as jacobi_table_system

MAX_DEGREE = 32


def coefficients(degree, lmin, lmax):
    """[c0, h_1, g_1, h_2, g_2, ...] in Python floats: the operations and their order are include/spmv_amd/api.h's."""
    theta = 0.5 * (lmax + lmin)
    delta = 0.5 * (lmax - lmin)
    sigma = theta / delta
    out = [1.0 / theta]
    rho = 1.0 / sigma
    for _ in range(degree):
        rho_next = 1.0 / (2.0 * sigma - rho)
        out.append(rho_next * rho)
        out.append(2.0 * rho_next / delta)
        rho = rho_next
    return out


def interval(A, dinv, lambda_min=0.0, lambda_max=0.0):
    """The library's rule: a bound > 0 is used as given, else lambda_max = the symmetric Gershgorin bound, lambda_min = lambda_max / 30."""
    hi = lambda_max if lambda_max > 0.0 else gershgorin(A, dinv)
    lo = lambda_min if lambda_min > 0.0 else hi / 30.0
    return lo, hi


def gershgorin(A, dinv):
    """max_i sum_j |a_ij| sqrt(|dinv_i| |dinv_j|), row i summed in CSR order from 0.0, one rounding per operation: the rows advance
    together slot by slot, so each row's sum is the sequential one."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    rows = A.shape[0]
    length = np.diff(A.indptr)
    sums = np.zeros(rows)
    ad = np.abs(np.asarray(dinv, dtype=np.float64))
    for k in range(int(length.max())):
        live = np.nonzero(length > k)[0]
        at = A.indptr[live] + k
        w = np.sqrt(ad[live] * ad[A.indices[at]])
        sums[live] = sums[live] + np.abs(A.data[at]) * w
    return float(np.max(sums))


def make_apply(matvec, dinv, coef, fma=None):
    """r -> z = M^-1 r. fma(a, x, y) = a * x + y rounded once (the oracle's axpy) makes it the kernels' arithmetic bit for bit, given
    matvec is the operator's own product; None: two roundings (numpy)."""
    if fma is None:
        def fma(a, x, y):
            return a * x + y
    degree = (len(coef) - 1) // 2

    def apply(r):
        u = dinv * r
        d = coef[0] * u
        z = d.copy()
        for k in range(1, degree + 1):
            h, g = coef[2 * k - 1], coef[2 * k]
            w = matvec(z)
            t = fma(-1.0, w, r)
            u = dinv * t
            d = fma(g, u, h * d)
            z = z + d
        return z

    return apply


def _loop(matvec, dot, b, x0, precond, tol, max_iters):
    """pcg_restatement._loop with z = precond(r)."""
    x = np.array(x0, dtype=np.float64)
    r = b - matvec(x)
    z = precond(r)
    p = z.copy()
    rz = dot(r, z)
    b_norm = float(np.sqrt(dot(r, r)))
    hist = [b_norm]
    it, converged = 0, False
    for _ in range(max_iters):
        Ap = matvec(p)
        pAp = dot(p, Ap)
        it += 1
        if pAp == 0.0 or not np.isfinite(pAp):
            hist.append(hist[-1])
            break
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        res = float(np.sqrt(dot(r, r)))
        hist.append(res)
        if res / b_norm < tol:
            converged = True
            break
        z = precond(r)
        rzn = dot(r, z)
        if rzn == 0.0 or not np.isfinite(rzn):
            break
        p = z + (rzn / rz) * p
        rz = rzn
    return x, np.array(hist), it, converged


def pcg(A, b, x0, degree, lo, hi, tol=1e-6, max_iters=1000):
    """Chebyshev-PCG with the interval given (the library's reported one, or interval()). Returns x, history, iterations, converged."""
    A = sp.csr_matrix(A)
    dinv = 1.0 / diagonal(A)
    mv = lambda v: A @ v
    return _loop(mv, lambda u, v: float(u @ v), b, x0, make_apply(mv, dinv, coefficients(degree, lo, hi)), tol, max_iters)


def pcg_other_rounding(A, b, x0, degree, lo, hi, tol=1e-6, max_iters=1000):
    """pcg() with every sum rounded differently (pcg_restatement.pcg_other_rounding): products through the CSC form, dot products in
    long double."""
    T = sp.csc_matrix(A)
    dinv = 1.0 / diagonal(A)
    ld = np.longdouble
    mv = lambda v: T @ v

    def dot(u, v):
        return float(np.sum(u.astype(ld) * v.astype(ld)))

    return _loop(mv, dot, b, x0, make_apply(mv, dinv, coefficients(degree, lo, hi)), tol, max_iters)


def table_system(name):
    """A, b, x0. "poisson<n>": stencil5(n, center=4.0) with rng = default_rng(n), b then x0 = rng.standard_normal(n * n); every other
    name is pcg_restatement.table_system's."""
    if name.startswith("poisson"):
        n = int(name[len("poisson"):])
        rng = np.random.default_rng(n)
        b = rng.standard_normal(n * n)
        x0 = rng.standard_normal(n * n)
        return stencil5(n, center=4.0), b, x0
    return jacobi_table_system(name)


# (system, degree, tol, iterations the CPU restatement takes in both roundings, automatic interval). degree None = Jacobi.
TABLE = [
    ("poisson127", None, 1e-6, 302), ("poisson127", 2, 1e-6, 107), ("poisson127", 4, 1e-6, 69), ("poisson127", 8, 1e-6, 45),
    ("poisson127", 4, 1e-10, 95),
    ("poisson255", None, 1e-6, 600), ("poisson255", 2, 1e-6, 212), ("poisson255", 4, 1e-6, 136), ("poisson255", 8, 1e-6, 89),
    ("poisson513", 4, 1e-6, 261),
    ("poisson640", 2, 1e-6, 509), ("poisson640", 8, 1e-6, 213),
    ("plain127", None, 1e-6, 19), ("plain127", 2, 1e-6, 13), ("plain127", 4, 1e-6, 8), ("plain127", 8, 1e-6, 5),
    ("plain601", None, 1e-6, 19), ("plain601", 2, 1e-6, 13), ("plain601", 4, 1e-6, 8), ("plain601", 8, 1e-6, 5),
    ("scaled127", None, 1e-6, 18), ("scaled127", 2, 1e-6, 13), ("scaled127", 4, 1e-6, 8), ("scaled127", 8, 1e-6, 5),
    ("negated65", None, 1e-6, 18), ("negated65", 2, 1e-6, 13), ("negated65", 4, 1e-6, 8), ("negated65", 8, 1e-6, 5),
    ("scaled601", None, 1e-6, 18), ("scaled601", 2, 1e-6, 13), ("scaled601", 4, 1e-6, 8), ("scaled601", 8, 1e-6, 5),
]
# the rows tests/test_chebyshev_host.py leaves out: 640^2 costs minutes on the CPU in two roundings
HOST_SKIPS = ("poisson640",)
