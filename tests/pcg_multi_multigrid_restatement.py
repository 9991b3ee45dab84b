"""numpy restatement of ONE column of the batched preconditioned solve under kind "multigrid" (csrc/pcg_multi.hip with the cycle of
csrc/multigrid_multi.hip). The loop is the one of pcg_multi_restatement.solve, restated here with the
preconditioner passed in: the dot products in the batched shape (pcg_multi_restatement.dot), the element-wise updates in the oracle's
fma forms, the scalar steps branch for branch. z = M^-1 r is multigrid_restatement.make_cycle on each level's own product (the
oracle's spmv_stencil5) with the oracle's fma: one V(nu, nu) cycle, steps (1)-(5) of include/spmv_amd/api.h. A column's result does
not depend on the batch it sits in, so one column is the whole statement. Test infrastructure: tests/test_mg_multi_host.py runs it on
the systems of multigrid_restatement.TABLE, tests/test_mg_multi_gpu.py compares applications and whole solves with it bit for bit."""
import numpy as np

import multi_rhs_restatement as M
import multigrid_restatement as MG
import pcg_multi_restatement as PM
from oracle import oracle as O


def level_products(levels):
    """Each level's product in the stencil operator's own order (the oracle's), from the restatement's level matrices."""
    out = []
    for L in levels:
        rp, ci, va = L.A.indptr.astype(np.int32), L.A.indices.astype(np.int32), np.ascontiguousarray(L.A.data)
        out.append(lambda v, rp=rp, ci=ci, va=va, n=L.n: O.spmv_stencil5(rp, ci, va, v, n))
    return out


def make_cycle(levels):
    """r -> z, one V-cycle, bit for bit the library's."""
    return MG.make_cycle(levels, level_products(levels), fma=O.axpy)


def solve_with(precond, matvec, pap_layout, b, x0, tol=1e-6, max_iters=1000):
    """One column under the preconditioner r -> z. Returns x, history (||r_k||, k = 0..iterations), iterations, converged, breakdown."""
    with np.errstate(all="ignore"):
        x = np.array(x0, dtype=np.float64)
        r = O.axpy(-1.0, matvec(x), b)           # fma(1.0, b, -1.0 * Ap): one rounding of b - Ap
        z = precond(r)
        p = z.copy()
        b_norm = float(np.sqrt(PM.dot(r, r)))
        rz = PM.dot(r, z)
        hist = [b_norm]
        it, converged, breakdown = 0, False, False
        for _ in range(max_iters):
            ap = matvec(p)
            pAp = PM.dot(p, ap, pap_layout)
            it += 1
            if not PM.usable(pAp):               # step 1: alpha = 0, skip_update; step 3: the residual of the r that stayed
                hist.append(float(np.sqrt(PM.dot(r, r))))
                breakdown = True
                break
            alpha = rz / pAp
            r = O.axpy(-alpha, ap, r)
            res = float(np.sqrt(PM.dot(r, r)))
            hist.append(res)
            if np.float64(res) / np.float64(b_norm) < tol:
                converged = True
                x = O.axpy(alpha, p, x)
                break
            z = precond(r)                       # the cycle: the device runs it whatever the verdict, its result is used here only
            rzn = PM.dot(r, z)
            if not PM.usable(rzn):               # step 4
                breakdown = True
                x = O.axpy(alpha, p, x)
                break
            beta = rzn / rz
            rz = rzn
            x = O.axpy(alpha, p, x)
            p = O.axpy(beta, p, z)
    return x, np.array(hist), it, converged, breakdown


def solve(A, n, b, x0, nu, tol=1e-6, max_iters=1000, max_levels=0, lambda_max=None):
    """One column on the n x n stencil A under the V(nu, nu) cycle of the automatic (or capped) hierarchy. lambda_max: the library's
    reported bounds, one per level, in place of the restatement's own. p.Ap is summed over the stencil SpMM's workgroups (256-column
    blocks of a grid row)."""
    levels = MG.hierarchy(MG.sorted_csr(A), n, nu, max_levels, lambda_max)
    products = level_products(levels)
    return solve_with(MG.make_cycle(levels, products, fma=O.axpy), products[0], M.grid(n), b, x0, tol, max_iters)
