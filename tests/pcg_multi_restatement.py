"""numpy restatement of ONE column of the batched preconditioned solve (csrc/pcg_multi.hip), read from the
kernels: the dot products in the batched shape -- the rounded product per row, 256 rows per partial (block_partials), the partials
through reduce_multi --, the element-wise updates in the oracle's fma forms, the scalar steps branch for branch. Given the operator's
own product (the oracle's spmv_*) it is the device's arithmetic bit for bit; a column's result does not depend on the batch it sits
in, so one column is the whole statement. Test infrastructure: tests/test_pcg_multi_host.py holds the dot against math.fsum and the
whole-solve systems against pcg_restatement / chebyshev_restatement, tests/test_pcg_multi_gpu.py compares solves with it bit for bit."""
import numpy as np

import chebyshev_restatement as CH
import multi_rhs_restatement as M
import reduction_restatement as RR
from oracle import oracle as O


def dot(u, v, layout=M.flat()):
    """A dot product of one column: r.r and r.z on flat 256-row workgroups; p.Ap on the SpMM's own (layout = its workgroups)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return RR.reduce_multi(M.block_partials_of(u * v, layout))


def usable(v):
    return v != 0.0 and np.isfinite(v)


def make_precond(matvec, dinv=None, coef=None):
    """r -> z. dinv None: kind "none"; coef None: "jacobi"; else "chebyshev" with coef = [c0, h_1, g_1, ...] (degree 0: c0 * (dinv * r))."""
    if dinv is None:
        return lambda r: r.copy()
    if coef is None:
        return lambda r: dinv * r
    return CH.make_apply(matvec, dinv, list(coef), fma=O.axpy)


def solve(matvec, pap_layout, b, x0, dinv=None, coef=None, tol=1e-6, max_iters=1000):
    """One column. Returns x, history (||r_k||, k = 0..iterations), iterations, converged, breakdown."""
    precond = make_precond(matvec, dinv, coef)
    with np.errstate(all="ignore"):
        x = np.array(x0, dtype=np.float64)
        r = O.axpy(-1.0, matvec(x), b)           # fma(1.0, b, -1.0 * Ap): one rounding of b - Ap
        z = precond(r)
        p = z.copy()
        b_norm = float(np.sqrt(dot(r, r)))
        rz = dot(r, z)
        hist = [b_norm]
        it, converged, breakdown = 0, False, False
        for _ in range(max_iters):
            ap = matvec(p)
            pAp = dot(p, ap, pap_layout)
            it += 1
            if not usable(pAp):                  # step 1: alpha = 0, skip_update; step 2 / 3: the residual of the r that stayed
                hist.append(float(np.sqrt(dot(r, r))))
                breakdown = True
                break
            alpha = rz / pAp
            r = O.axpy(-alpha, ap, r)
            res = float(np.sqrt(dot(r, r)))
            hist.append(res)
            if np.float64(res) / np.float64(b_norm) < tol:
                converged = True
                x = O.axpy(alpha, p, x)
                break
            z = precond(r)
            rzn = dot(r, z)
            if not usable(rzn):
                breakdown = True
                x = O.axpy(alpha, p, x)
                break
            beta = rzn / rz
            rz = rzn
            x = O.axpy(alpha, p, x)
            p = O.axpy(beta, p, z)
    return x, np.array(hist), it, converged, breakdown


def solve_numpy(A, b, x0, dinv=None, coef=None, tol=1e-6, max_iters=1000):
    """solve() on a scipy matrix with numpy forms (a * x + y rounds twice): the batched dot shape on pcg_restatement's loop. What the
    host test compares with pcg() to show the dot shape moves no iteration count."""
    mv = lambda v: A @ v
    if dinv is None:
        precond = lambda r: r
    elif coef is None:
        precond = lambda r: dinv * r
    else:
        precond = CH.make_apply(mv, dinv, list(coef))
    return CH._loop(mv, lambda u, v: dot(u, v), b, x0, precond, tol, max_iters)
