"""numpy restatement of ONE column of the batched preconditioned solve under kind "multigrid" on the 3-D operator (csrc/pcg_multi.hip
with the cycle of csrc/multigrid_multi.hip on the launches of csrc/multigrid3d_multi.hip). The loop is
pcg_multi_multigrid_restatement.solve_with itself; z = M^-1 r is multigrid3d_restatement.make_cycle on multigrid3d_restatement's
hierarchy, every level's product the CSR loop (the oracle's spmv_csr) and the oracle's fma: one V(nu, nu) cycle, steps (1)-(5) of
include/spmv_amd/api.h. p.Ap is summed over the workgroups of the operator's own SpMM on stencil7-csr, "spmm/csr": 256 flat rows each.
A column's result does not depend on the batch it sits in, so one column is the whole statement. Test infrastructure:
tests/test_mg3d_multi_host.py runs it on the rows of multigrid3d_restatement.TABLE with n <= 33, tests/test_mg3d_multi_gpu.py compares
applications and whole solves with it bit for bit."""
import numpy as np

import multi_rhs_restatement as M
import multigrid3d_restatement as M3
import pcg_multi_multigrid_restatement as MM
from oracle import oracle as O


def level_products(levels):
    """Each level's product in the operator's own order: the CSR loop, every row."""
    out = []
    for L in levels:
        rp, ci, va = L.A.indptr.astype(np.int32), L.A.indices.astype(np.int32), np.ascontiguousarray(L.A.data)
        out.append(lambda v, rp=rp, ci=ci, va=va: O.spmv_csr(rp, ci, va, v))
    return out


def make_cycle(levels):
    """r -> z, one V-cycle, bit for bit the library's."""
    return M3.make_cycle(levels, level_products(levels), fma=O.axpy)


def solve_levels(levels, b, x0, tol=1e-6, max_iters=1000):
    """One column on a hierarchy already built (level 0 holds the system's matrix)."""
    products = level_products(levels)
    return MM.solve_with(M3.make_cycle(levels, products, fma=O.axpy), products[0], M.flat(), b, x0, tol, max_iters)


def solve(A, n, b, x0, nu, tol=1e-6, max_iters=1000, max_levels=0, lambda_max=None):
    """One column on the n^3 stencil A under the V(nu, nu) cycle of the automatic (or capped) hierarchy. lambda_max: the library's
    reported bounds, one per level, in place of the restatement's own."""
    return solve_levels(M3.hierarchy(M3.sorted_csr(A), n, nu, max_levels, lambda_max), b, x0, tol, max_iters)
