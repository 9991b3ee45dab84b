"""numpy restatement of ONE column of the batched solves under an aggregation AMG hierarchy with block vectors
(spmv_amd_precond_create_amg_multi: csrc/amg_multi.hip with the cycle of csrc/multigrid_multi.hip). The hierarchy
and the cycle are amg_restatement's; what the batched cycle changes is stated in include/spmv_amd/api.h: EVERY level's product is the
sequential chain s = +0.0 ; s = fma(v[k], z[col[k]], s) (the oracle's spmv_csr, what "spmm/csr" computes), under the smoother as under
the restriction, and every update is the oracle's fma. The PCG loop is pcg_multi_multigrid_restatement.solve_with itself, p.Ap summed
over the workgroups of the operator's own SpMM on cusparse-csr, "spmm/csr": 256 flat rows each; the GCR column is
gcr_multi_restatement's loop with the cycle as the application. A column's result does not depend on the batch it sits in, so one
column is the whole statement. Test infrastructure: tests/test_amg_multi_host.py runs it on rows of amg_restatement.TABLE,
tests/test_amg_multi_gpu.py compares applications and whole solves with it bit for bit."""
import amg_restatement as AMG
import csr_restatement as CSR
import gcr_multi_restatement as GM
import multi_rhs_restatement as M
import pcg_multi_multigrid_restatement as MM
from oracle import oracle as O


def chains(levels):
    """Each level's product as the sequential chain, every row."""
    return [(lambda v, L=L: O.spmv_csr(L.M.rp, L.M.ci, L.M.va, v)) for L in levels]


def make_cycle(levels):
    """r -> z, one V-cycle, bit for bit the batched library's."""
    products = chains(levels)
    return AMG.make_cycle(levels, products, products, fma=O.axpy)


def level_variants(levels):
    """The variant every level's SINGLE-vector product runs (level 0: the operator's automatic one): where all are "stream" or
    "row-scalar" the single handle's bits are the batched ones."""
    return [CSR.variant_of(L.M.rp, None) for L in levels]


def bits_coincide(levels):
    return all(v in ("stream", "row-scalar") for v in level_variants(levels))


def solve_levels(levels, b, x0, tol=1e-6, max_iters=1000):
    """One PCG column on a hierarchy already built (level 0 holds the system's matrix). Returns x, history, iterations, converged,
    breakdown."""
    return MM.solve_with(make_cycle(levels), chains(levels)[0], M.flat(), b, x0, tol, max_iters)


def gcr_levels(levels, b, x0, restart=0, tol=1e-6, max_iters=1000):
    """One GCR(restart) column. Returns x, history, iterations, converged, how it ended."""
    return GM.solve(chains(levels)[0], b, x0, make_cycle(levels), restart, tol, max_iters)
