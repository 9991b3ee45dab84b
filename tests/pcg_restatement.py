"""numpy restatement of the preconditioned CG loop of spmv_amd_pcg_solve_device (csrc/pcg.hip) and the
matrices its tests use. dinv = None means kind "none" (z = r)."""
import numpy as np
import scipy.sparse as sp

ENTRY_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("value", np.float64)], align=True)


def stencil5(n, center=5.0, off=-1.0):
    """The benchmark's 5-point stencil on an n x n grid (scipy CSR)."""
    t = sp.diags([np.full(n - 1, off), np.full(n, center), np.full(n - 1, off)], [-1, 0, 1])
    eye = sp.identity(n)
    lap = sp.kron(eye, t) + sp.kron(sp.diags([np.full(n - 1, off), np.full(n - 1, off)], [-1, 1]), eye)
    return sp.csr_matrix(lap)


def scaled_stencil5(n, decades, seed):
    """S A S with s_i = 10^U(0, decades): SPD, diagonal varying over 2 * decades orders of magnitude."""
    s = 10.0 ** np.random.default_rng(seed).uniform(0.0, decades, n * n)
    S = sp.diags(s)
    return sp.csr_matrix(S @ stencil5(n) @ S)


def entries_of(A):
    """COO entries (row-major order) of a scipy matrix, in the library's MatrixData layout."""
    c = sp.coo_matrix(A)
    order = np.lexsort((c.col, c.row))
    e = np.zeros(len(order), dtype=ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = c.row[order], c.col[order], c.data[order]
    return e


def diagonal(A):
    """d_i as the library defines it: the sum of row i's entries in column i."""
    return np.asarray(sp.csr_matrix(A).diagonal(), dtype=np.float64)


def _loop(matvec, dot, b, x0, dinv, tol, max_iters):
    x = np.array(x0, dtype=np.float64)
    r = b - matvec(x)
    z = r if dinv is None else dinv * r
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
        z = r if dinv is None else dinv * r
        rzn = dot(r, z)
        if rzn == 0.0 or not np.isfinite(rzn):
            break
        p = z + (rzn / rz) * p
        rz = rzn
    return x, np.array(hist), it, converged


def pcg(A, b, x0, dinv, tol=1e-6, max_iters=1000):
    """Returns x, history (||r_k||, k = 0..iterations), iterations, converged."""
    return _loop(lambda v: A @ v, lambda u, v: float(u @ v), b, x0, dinv, tol, max_iters)


def pcg_other_rounding(A, b, x0, dinv, tol=1e-6, max_iters=1000):
    """pcg() with every sum rounded differently: the product through the CSC form of A (each y_i accumulated in column order,
    not row order) and the dot products in long double. What the two disagree by on an input is what a comparison against
    either at 1e-10 can mean on that input (tests/test_pcg_host.py keeps the table)."""
    T = sp.csc_matrix(A)
    ld = np.longdouble

    def dot(u, v):
        return float(np.sum(u.astype(ld) * v.astype(ld)))

    return _loop(lambda v: T @ v, dot, b, x0, dinv, tol, max_iters)


def true_residual_norm(entries, b, x):
    """||b - A x|| accumulated in long double from the COO entries: no algebra shared with the CG recurrences."""
    ld = np.longdouble
    r = np.asarray(b, dtype=np.float64).astype(ld)
    np.subtract.at(r, entries["row"], entries["value"].astype(ld) * np.asarray(x, dtype=np.float64).astype(ld)[entries["col"]])
    return float(np.sqrt(np.sum(r * r)))


# The systems of the whole-solve tests beyond x0 = 0 (tests/test_pcg_gpu.py): name -> (matrix, seed of b and x0). Chosen so
# that pcg() and pcg_other_rounding() agree far below the tests' 1e-10 (tests/test_pcg_host.py re-runs that comparison).
def table_system(name):
    """Returns A, b, x0 of one system of the table: rng = default_rng(seed), b then x0 = rng.standard_normal(rows)."""
    n, decades, seed, sign = {"scaled127": (127, 2, 11, 1.0), "negated65": (65, 1, 12, -1.0), "scaled600": (600, 1, 13, 1.0),
                              "scaled601": (601, 2, 14, 1.0), "plain127": (127, 0, 127, 1.0), "plain601": (601, 0, 601, 1.0)}[name]
    A = stencil5(n) if decades == 0 else sp.csr_matrix(sign * scaled_stencil5(n, decades, seed))
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n * n)
    x0 = rng.standard_normal(n * n)
    return A, b, x0


# (system, kind, tol, max_iters, iterations the CPU restatement takes in both roundings)
TABLE = [
    ("scaled127", "jacobi", 1e-6, 1000, 18), ("scaled127", "jacobi", 1e-10, 1000, 31),
    ("negated65", "jacobi", 1e-6, 1000, 18), ("negated65", "jacobi", 1e-10, 1000, 32),
    ("scaled600", "jacobi", 1e-6, 1000, 19), ("scaled600", "jacobi", 1e-10, 1000, 32),
    ("scaled600", "none", 1e-6, 1000, 92),
    ("scaled601", "jacobi", 1e-6, 1000, 18), ("scaled601", "jacobi", 1e-10, 1000, 31),
    ("plain127", "none", 1e-6, 1000, 19), ("plain127", "jacobi", 1e-6, 1000, 19),
    ("plain127", "none", 1e-10, 1000, 33), ("plain127", "jacobi", 1e-10, 1000, 33),
    ("plain601", "none", 1e-6, 1000, 19), ("plain601", "jacobi", 1e-6, 1000, 19),
    ("plain601", "none", 1e-10, 1000, 33), ("plain601", "jacobi", 1e-10, 1000, 33),
    ("scaled127", "none", 1e-6, 40, 40),  # kind none on a scaled matrix: only its first 40 residuals are a property of the input
]


def hist_err(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.asarray(want)))
