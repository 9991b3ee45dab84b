"""numpy restatement of ONE column of the batched GCR(m) solve (csrc/gcr_multi.hip): the loop of
gcr_restatement._loop -- the algebra of api.h step for step, classical Gram-Schmidt from the q of the product, i ascending, the two
breakdowns, the strict stopping test -- with every dot product in the batched shape (pcg_multi_restatement.dot on flat 256-row
workgroups: the rounded product per row, block_partials, the two reduction stages) and every update through the oracle's fma. Given
the operator's own product (the oracle's spmv_*) and the application in the library's bits (gcr_restatement.exact_apply on the CPU;
the GPU tests hand in spmv_amd_precond_apply_device_multi, which the block applications' own tests hold bit for bit) it is the
device's arithmetic bit for bit; a column's result depends neither on the batch it sits in nor on its slot, so one column is the whole
statement. The columns are bicgstab_multi_restatement's: seed 0 is the table system, seeds 1..8 its seeded columns.
Test infrastructure: tests/test_gcr_multi_host.py holds it against the two CPU roundings of gcr_restatement and computes the table's
figures, tests/test_gcr_multi_gpu.py compares solves with it bit for bit."""
import functools

import numpy as np

import bicgstab_multi_restatement as BM
import gcr_restatement as GR
import pcg_multi_restatement as PM
from bicgstab_multi_restatement import batch, seeded_column  # noqa: F401

TOL = 1e-6  # of every table row


def solve(matvec, b, x0, apply, restart=0, tol=TOL, max_iters=1000):
    """One column on the operator's own product and the library's application. Returns x, history, iterations, converged and how it
    ended ("converged", "gamma", "rho" or "max_iters")."""
    from oracle import oracle as O

    def fma(a, u, c):
        return O.fma(np.full(len(u), a), u, c)

    with np.errstate(all="ignore"):
        return GR._loop(matvec, PM.dot, b, x0, apply, restart, tol, max_iters, fma)


def solve_numpy(A, b, x0, apply, restart=0, tol=TOL, max_iters=1000):
    """solve() on a scipy matrix with numpy forms (a * b + c rounds twice): the batched dot shape alone on gcr()'s loop."""
    with np.errstate(all="ignore"):
        return GR._loop(lambda u: A @ u, PM.dot, b, x0, apply, restart, tol, max_iters)


def column(name, seed):
    """b, x0 of column `seed` of a table system: 0 is the system's own pair, 1..8 the seeded columns."""
    if seed == 0:
        _, b, x0 = GR.table_system(name)
        return b, x0
    return BM.seeded_column(name, seed)


@functools.lru_cache(maxsize=None)
def two_roundings(name, kind, restart, seed, tol=TOL):
    """One table row in plain numpy and in the other rounding (gcr_restatement.gcr / gcr_other_rounding)."""
    A, _, _ = GR.table_system(name)
    b, x0 = column(name, seed)
    dim = GR.dimension_of(name)
    return (GR.gcr(A, b, x0, GR.make_apply(A, dim, kind), restart, tol),
            GR.gcr_other_rounding(A, b, x0, GR.make_apply(A, dim, kind, csc=True), restart, tol))


# (system, kind, restart, seed) -> (iterations both CPU roundings take at tol 1e-6, how both end, their largest relative history
# disagreement: stored as twice what tests/test_gcr_multi_host.py measures, which it prints, and never below 1e-14 -- the factor and
# the floor of gcr_restatement.TABLE). Another rounding of a row -- the restatement here, the device, the single-RHS solver -- is held
# against plain numpy to gcr_restatement.third_rounding_bound(stored). Every (system, kind, restart) the whole-solve GPU tests run is
# here with seeds 0..7, the columns of a batch of 8; no row had to be dropped: on each both roundings agree on count and end.
TABLE = {
    ("grid33", "none", 1, 0): (101, "converged", 1e-14), ("grid33", "none", 1, 1): (99, "converged", 1e-14),
    ("grid33", "none", 1, 2): (97, "converged", 1e-14), ("grid33", "none", 1, 3): (103, "converged", 1e-14),
    ("grid33", "none", 1, 4): (104, "converged", 1e-14), ("grid33", "none", 1, 5): (96, "converged", 1e-14),
    ("grid33", "none", 1, 6): (90, "converged", 1e-14), ("grid33", "none", 1, 7): (94, "converged", 1e-14),
    ("grid33", "none", 4, 0): (49, "converged", 1e-14), ("grid33", "none", 4, 1): (49, "converged", 1e-14),
    ("grid33", "none", 4, 2): (47, "converged", 1e-14), ("grid33", "none", 4, 3): (49, "converged", 1e-14),
    ("grid33", "none", 4, 4): (51, "converged", 1e-14), ("grid33", "none", 4, 5): (48, "converged", 1e-14),
    ("grid33", "none", 4, 6): (48, "converged", 1e-14), ("grid33", "none", 4, 7): (49, "converged", 1e-14),
    ("grid33", "jacobi", 16, 0): (48, "converged", 1e-14), ("grid33", "jacobi", 16, 1): (48, "converged", 1e-14),
    ("grid33", "jacobi", 16, 2): (47, "converged", 5e-14), ("grid33", "jacobi", 16, 3): (48, "converged", 1e-14),
    ("grid33", "jacobi", 16, 4): (50, "converged", 9e-14), ("grid33", "jacobi", 16, 5): (48, "converged", 6e-14),
    ("grid33", "jacobi", 16, 6): (47, "converged", 2e-14), ("grid33", "jacobi", 16, 7): (48, "converged", 2e-14),
    ("grid33", "chebyshev2", 4, 0): (44, "converged", 3e-13), ("grid33", "chebyshev2", 4, 1): (45, "converged", 2e-14),
    ("grid33", "chebyshev2", 4, 2): (45, "converged", 2e-13), ("grid33", "chebyshev2", 4, 3): (47, "converged", 8e-14),
    ("grid33", "chebyshev2", 4, 4): (40, "converged", 5e-14), ("grid33", "chebyshev2", 4, 5): (47, "converged", 2e-14),
    ("grid33", "chebyshev2", 4, 6): (46, "converged", 9e-14), ("grid33", "chebyshev2", 4, 7): (45, "converged", 6e-14),
    ("grid33", "multigrid1", 16, 0): (10, "converged", 1e-14), ("grid33", "multigrid1", 16, 1): (10, "converged", 1e-14),
    ("grid33", "multigrid1", 16, 2): (10, "converged", 1e-14), ("grid33", "multigrid1", 16, 3): (10, "converged", 1e-14),
    ("grid33", "multigrid1", 16, 4): (10, "converged", 1e-14), ("grid33", "multigrid1", 16, 5): (10, "converged", 1e-14),
    ("grid33", "multigrid1", 16, 6): (9, "converged", 1e-14), ("grid33", "multigrid1", 16, 7): (10, "converged", 1e-14),
    ("grid65", "none", 16, 0): (61, "converged", 1e-14), ("grid65", "none", 16, 1): (61, "converged", 1e-14),
    ("grid65", "none", 16, 2): (60, "converged", 1e-14), ("grid65", "none", 16, 3): (60, "converged", 1e-14),
    ("grid65", "none", 16, 4): (60, "converged", 1e-14), ("grid65", "none", 16, 5): (62, "converged", 1e-14),
    ("grid65", "none", 16, 6): (62, "converged", 1e-14), ("grid65", "none", 16, 7): (61, "converged", 1e-14),
    ("grid65", "multigrid1", 4, 0): (11, "converged", 3e-14), ("grid65", "multigrid1", 4, 1): (11, "converged", 2e-14),
    ("grid65", "multigrid1", 4, 2): (11, "converged", 4e-14), ("grid65", "multigrid1", 4, 3): (12, "converged", 1e-14),
    ("grid65", "multigrid1", 4, 4): (11, "converged", 3e-14), ("grid65", "multigrid1", 4, 5): (11, "converged", 3e-14),
    ("grid65", "multigrid1", 4, 6): (12, "converged", 4e-14), ("grid65", "multigrid1", 4, 7): (11, "converged", 4e-14),
    ("cube16", "none", 4, 0): (39, "converged", 1e-14), ("cube16", "none", 4, 1): (40, "converged", 1e-14),
    ("cube16", "none", 4, 2): (39, "converged", 1e-14), ("cube16", "none", 4, 3): (41, "converged", 1e-14),
    ("cube16", "none", 4, 4): (42, "converged", 1e-14), ("cube16", "none", 4, 5): (41, "converged", 2e-14),
    ("cube16", "none", 4, 6): (41, "converged", 1e-14), ("cube16", "none", 4, 7): (40, "converged", 1e-14),
    ("cube16", "chebyshev2", 16, 0): (28, "converged", 1e-12), ("cube16", "chebyshev2", 16, 1): (28, "converged", 3e-12),
    ("cube16", "chebyshev2", 16, 2): (27, "converged", 3e-12), ("cube16", "chebyshev2", 16, 3): (26, "converged", 5e-13),
    ("cube16", "chebyshev2", 16, 4): (28, "converged", 4e-13), ("cube16", "chebyshev2", 16, 5): (28, "converged", 1e-12),
    ("cube16", "chebyshev2", 16, 6): (28, "converged", 8e-12), ("cube16", "chebyshev2", 16, 7): (28, "converged", 8e-13),
    ("cube16", "multigrid1", 4, 0): (7, "converged", 1e-14), ("cube16", "multigrid1", 4, 1): (7, "converged", 4e-14),
    ("cube16", "multigrid1", 4, 2): (7, "converged", 1e-14), ("cube16", "multigrid1", 4, 3): (8, "converged", 1e-14),
    ("cube16", "multigrid1", 4, 4): (8, "converged", 2e-14), ("cube16", "multigrid1", 4, 5): (8, "converged", 2e-14),
    ("cube16", "multigrid1", 4, 6): (8, "converged", 1e-14), ("cube16", "multigrid1", 4, 7): (7, "converged", 3e-13),
}
# The (system, kind, restart) of the table, in its order.
CASES = sorted({key[:3] for key in TABLE}, key=lambda c: next(i for i, key in enumerate(TABLE) if key[:3] == c))


def rows_of(name, kind, restart):
    return [(seed, TABLE[(name, kind, restart, seed)]) for seed in range(8)]
