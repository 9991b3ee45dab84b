"""numpy restatement of ONE column of the batched BiCGSTAB solve (csrc/bicgstab_multi.hip): the loop of
bicgstab_restatement._loop -- the algebra of api.h step for step, the half step, the three breakdowns, the strict stopping test --
with every dot product in the batched shape (pcg_multi_restatement.dot on flat 256-row workgroups: the rounded product per row,
block_partials, the two reduction stages) and every update through the oracle's fma. Given the operator's own product (the oracle's
spmv_*) it is the device's arithmetic bit for bit; a column's result depends neither on the batch it sits in nor on its slot, so one
column is the whole statement. Test infrastructure: tests/test_bicgstab_multi_host.py holds it against the two CPU roundings of
bicgstab_restatement and pins the seeded columns, tests/test_bicgstab_multi_gpu.py compares solves with it bit for bit."""
import functools

import numpy as np

import bicgstab_restatement as BR
import pcg_multi_restatement as PM

TOL = 1e-6  # of the seeded columns


def solve(matvec, b, x0, dinv=None, tol=TOL, max_iters=1000):
    """One column on the operator's own product. Returns x, history, iterations, converged and how it ended ("half", "whole", "sigma",
    "omega", "rho" or "max_iters")."""
    from oracle import oracle as O

    def fma(a, u, c):
        return O.fma(np.full(len(u), a), u, c)

    with np.errstate(all="ignore"):
        return BR._loop(matvec, PM.dot, b, x0, dinv, tol, max_iters, fma)


def solve_numpy(A, b, x0, dinv=None, tol=TOL, max_iters=1000):
    """solve() on a scipy matrix with numpy forms (a * b + c rounds twice): the batched dot shape alone on bicgstab()'s loop."""
    with np.errstate(all="ignore"):
        return BR._loop(lambda u: A @ u, PM.dot, b, x0, dinv, tol, max_iters)


@functools.lru_cache(maxsize=None)
def seeded_column(name, s):
    """b, x0 of extra column s = 1..8 of a table system: rng = default_rng(1000 + s), b then x0 = rng.standard_normal(rows)."""
    rows = BR.table_system(name)[0].shape[0]
    rng = np.random.default_rng(1000 + s)
    b = rng.standard_normal(rows)
    x0 = rng.standard_normal(rows)
    return b, x0


def batch(name, k):
    """B, X0 (k, rows): column 0 is the table system, columns 1 .. k - 1 the seeded columns 1 .. k - 1."""
    _, b, x0 = BR.table_system(name)
    cols = [(b, x0)] + [seeded_column(name, s) for s in range(1, k)]
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols])


# What the exact restatement gives on seeded column s = 1..8 at tol 1e-6, the same for kinds "none" and "jacobi" and in the two CPU
# roundings (tests/test_bicgstab_multi_host.py holds all of that): (iterations, end) per column.
SEEDED = {
    "grid33": [(30, "half"), (27, "whole"), (32, "half"), (29, "whole"), (29, "half"), (27, "whole"), (27, "half"), (28, "half")],
    "grid65": [(34, "half"), (32, "whole"), (33, "whole"), (33, "whole"), (36, "half"), (35, "whole"), (35, "half"), (34, "half")],
    "cube16": [(23, "half"), (22, "whole"), (24, "half"), (26, "half"), (29, "half"), (25, "whole"), (26, "whole"), (22, "whole")],
}
