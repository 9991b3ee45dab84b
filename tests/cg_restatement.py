"""numpy restatement of the CG loop of csrc/cg_slab_solve.hip (the slab solver and, through it, cg_solve_device), every bit specified:
A p by the oracle's SpMV, the updates of r, p, x by the oracle's element-wise forms (oracle_cg_partitioned's arithmetic), the three
dot products by tests/reduction_restatement.py and the scalar step of cg_scalars_step (csrc/reduce_device.hpp):
alpha = rr_old / pAp, beta = rr_new / rr_old, converged when sqrt(rr_new) / b_norm < tol, strictly. Test infrastructure
(tests/test_cg_restated_gpu.py)."""
import numpy as np

import reduction_restatement as R
from oracle import oracle as O


class System:
    """What a solve needs to know about its operator: spmv(v) -> A v; pap(p, Ap) and rr0(r0) -> (partials, extras) as the
    launches write them; device_form: p = fma(beta, p, r) (cg_solve_device) instead of fma(1, r, beta * p) (the slab solver)."""

    def __init__(self, spmv, pap, rr0, device_form=False):
        self.spmv, self.pap, self.rr0, self.device_form = spmv, pap, rr0, device_form


def stream_rr0(r0):
    """SpMV on x0, then cg_init_residual_kernel (slabs and operators without the fused initial residual)"""
    return R.residual_partials(r0), ()


def whole_grid(O_, rp, ci, va, n, form, device_form=False):
    """One rank, the whole n x n grid. form: "row-direct" | "row-lds" (the fused initial residual comes with it)."""
    spmv = lambda v: O_.spmv_stencil5(rp, ci, va, v, n)  # noqa: E731
    if form == "row-lds":
        return System(spmv, lambda p, ap: (R.rowlds_partials(p, ap, n), ()), lambda r0: (R.rowlds_partials(r0, r0, n), ()), device_form)
    assert form == "row-direct"
    return System(spmv, lambda p, ap: (R.rowdirect_partials(p, ap, n), ()), stream_rr0, device_form)


def ellpack(O_, rp, ci, va):
    """cg_solve_device on the ELLPACK operator: the fused p.Ap of ell_block_dot, r0 by the streaming kernel."""
    rows = len(rp) - 1
    width, idx, val = O_.build_ell(rp, ci, va)
    return System(lambda v: O_.spmv_ell(rows, width, idx, val, v), lambda p, ap: (R.ell_partials(p, ap), ()), stream_rr0, True)


def stand_in(O_, n, as_rank, as_world):
    """Rank as_rank of as_world of the n x n stencil on one self-neighbour rank (tests/test_distributed.py, stand_in_system): the
    halo rows hold the slab's own first / last grid row. Row-lds; the rows that read a halo -- the first grid row of a slab with a
    previous rank, the last of one with a next rank -- are evaluated behind the interior rows and their tiles' partials enter
    the sum as extras, first grid row before last (slab_boundary_spmv, launch_stencil5_edges_and_reduce)."""
    off, nl = O_.partition_rows(n * n, as_world, as_rank)
    rp, ci, va = O_.stencil5_csr(n)
    base = rp[off]
    lrp = (rp[off:off + nl + 1] - base).astype(np.int32)
    lci, lva = ci[base:], va[base:]
    prev, nxt = as_rank > 0, as_rank < as_world - 1

    def spmv(v):
        return O_.spmv_halo(lrp, lci, lva, v, v[:n] if prev else None, v[nl - n:] if nxt else None, off, n * n, n)

    def split(a, s):
        lo, hi = (n if prev else 0), nl - (n if nxt else 0)
        extras = [R.rowlds_partials(a[:n], s[:n], n)] if prev else []
        if nxt:
            extras.append(R.rowlds_partials(a[hi:], s[hi:], n))
        return R.rowlds_partials(a[lo:hi], s[lo:hi], n), np.concatenate(extras) if extras else ()

    return System(spmv, split, lambda r0: split(r0, r0)), off, nl


def solve(system, b, x0, max_iters, tol):
    """Returns x, the residual history (||r0||, then one entry per iteration), the iteration count and the verdict."""
    b, x = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(x0, dtype=np.float64).copy()
    r = O.axpy(-1.0, system.spmv(x), b)  # fma(-1, A x0, b)
    p = r.copy()
    rr_old = R.reduce(*system.rr0(r))
    b_norm = np.sqrt(np.float64(rr_old))
    history, iterations, converged = [float(b_norm)], 0, 0
    while iterations < max_iters:
        ap = system.spmv(p)
        p_ap = R.reduce(*system.pap(p, ap))
        alpha = float(np.float64(rr_old) / np.float64(p_ap))
        r = O.axpy(-alpha, ap, r)
        rr_new = R.reduce(R.residual_partials(r))
        x = O.axpy(alpha, p, x)
        iterations += 1
        history.append(float(np.sqrt(np.float64(rr_new))))
        if np.sqrt(np.float64(rr_new)) / b_norm < tol:
            converged = 1
            break
        beta = float(np.float64(rr_new) / np.float64(rr_old))
        rr_old = rr_new
        p = O.update_p(r, beta, p) if system.device_form else O.axpby(1.0, r, beta, p)
    return x, np.array(history), iterations, converged
