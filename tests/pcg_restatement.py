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


def pcg(A, b, x0, dinv, tol=1e-6, max_iters=1000):
    """Returns x, history (||r_k||, k = 0..iterations), iterations, converged."""
    x = np.array(x0, dtype=np.float64)
    r = b - A @ x
    z = r if dinv is None else dinv * r
    p = z.copy()
    rz = float(r @ z)
    b_norm = float(np.sqrt(r @ r))
    hist = [b_norm]
    it, converged = 0, False
    for _ in range(max_iters):
        Ap = A @ p
        pAp = float(p @ Ap)
        it += 1
        if pAp == 0.0 or not np.isfinite(pAp):
            hist.append(hist[-1])
            break
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        res = float(np.sqrt(r @ r))
        hist.append(res)
        if res / b_norm < tol:
            converged = True
            break
        z = r if dinv is None else dinv * r
        rzn = float(r @ z)
        if rzn == 0.0 or not np.isfinite(rzn):
            break
        p = z + (rzn / rz) * p
        rz = rzn
    return x, np.array(hist), it, converged


def hist_err(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.asarray(want)))
