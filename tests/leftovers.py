"""A clean solve on the remains of a solve that ended badly (tests/test_leftovers_host.py, tests/test_leftovers_gpu.py). Test
infrastructure only.

Every solver keeps device state between calls -- vectors, direction-ring slots with their alpha slots, basis slots, partials, slice
tickets, the scalar record or the per-column records, a history buffer that only grows -- and re-makes it only when the size, the
device or the batch width changes. A stale value that is read and multiplied by 0, or read only in the converging or the run-ahead
iteration, changes no bit after a finite predecessor; after a NaN predecessor it is a NaN in x. A stale stop / done / skip_update
flag shows only after a predecessor that set it. This module is the table of such predecessors (DIRTY), the clean solves that follow
them (CLEAN) and the one harness that runs the pair: dirty_then_clean().

A solve is described, not held: Solve(name, rhs, x0, tol, max_iters, variant). vectors() turns the description into b and x0 for a
grid. `variant` is the subject's own: None = the subject's kind / restart / degree, anything else = the other one to run under on the
same workspace (the other_kind rows)."""
import collections
import functools

import numpy as np

import poison
from bitwise import same_bits

Solve = collections.namedtuple("Solve", "name rhs x0 tol max_iters variant", defaults=(None,))
# one column of a result; `breakdown` is None where the statistics of the family have no such field
Column = collections.namedtuple("Column", "x history iterations converged breakdown residual_norm")

RING, RESTART, BASIS = 16, 16, 32  # the longest direction ring, the default restart, the basis slots GCR can hold
SHORT, LONG, NAN_ITERS, HUGE_ITERS = 3, 40, 20, 2 * BASIS + 5
CONVERGING_TOL, CONVERGING_CAP = 1e-8, 400
EARLY_TOL = 0.1
SENTINEL = -7.25e77  # what a history buffer is pre-filled with: no residual norm is negative
HISTORY_SLACK = 24   # entries of a history buffer behind the longest history it could be handed

# counts are fixed by max_iters at tol = 0: nothing needs measuring
CLEAN = [Solve(f"{name}-x0{x0}", "normal", x0, tol, cap)
         for name, tol, cap in (("short", 0.0, SHORT), ("long", 0.0, LONG), ("converging", CONVERGING_TOL, CONVERGING_CAP))
         for x0 in ("zero", "nonzero")]
DIRTY = [
    Solve("nan_b", "nan", "nonzero", 0.0, NAN_ITERS),        # plain CG runs all 20, past a 16-slot ring; a breakdown rule stops at 1
    Solve("inf_b", "inf_seams", "nonzero", 0.0, NAN_ITERS),  # +inf at the seam columns of two grid rows
    Solve("zero_b", "zero", "zero", CONVERGING_TOL, NAN_ITERS),
    Solve("no_iterations", "normal", "nonzero", 0.0, 0),
    Solve("huge_long", "huge", "nonzero", 0.0, HUGE_ITERS),  # finite junk of another magnitude in every slot, the longest history
    # beside the rows above, which all end unconverged: a predecessor that sets the converged / done flags, early in its ring or restart
    Solve("early_stop", "normal", "nonzero", EARLY_TOL, CONVERGING_CAP),
]
assert SHORT < 4 and LONG > 2 * RING and LONG > 2 * RESTART and HUGE_ITERS > 2 * BASIS and HUGE_ITERS > LONG


def other_kind(variant, max_iters=NAN_ITERS):
    """The same family under another kind, restart or degree on the same workspace: an ordinary capped solve."""
    return Solve(f"other_kind-{variant}", "normal", "nonzero", 0.0, max_iters, variant)


def dirties(*variants):
    """The table's dirtying solves and one other_kind row per variant of the subject."""
    return DIRTY + [other_kind(v) for v in variants]


def inf_rows(grid, dim):
    """The rows inf_b poisons: poison.seam_columns of grid row 1 and of the middle grid row (dim 3: of the first plane)."""
    cols = np.array(poison.seam_columns(grid), dtype=np.int64)
    return np.concatenate([g * grid + cols for g in (1, grid // 2)])


def vectors(solve, grid, dim=2, seed=0):
    """b, x0 of a described solve on the grid^dim system: fresh arrays, seeded by (grid, dim, seed) alone, so that every solve of a
    table has the same "normal" b and the same non-zero x0."""
    rows = grid ** dim
    rng = np.random.default_rng(77000 + 100 * grid + 10 * dim + seed)
    normal, start, junk = rng.standard_normal(rows), 0.1 * rng.standard_normal(rows), rng.standard_normal(rows)
    if solve.rhs == "normal":
        b = normal
    elif solve.rhs == "nan":
        b = np.full(rows, np.nan)
    elif solve.rhs == "inf_seams":
        b = normal.copy()
        b[inf_rows(grid, dim)] = np.inf
    elif solve.rhs == "zero":
        b = np.zeros(rows)
    else:
        assert solve.rhs == "huge", solve.rhs
        b = 1e100 * junk
    return b, (np.zeros(rows) if solve.x0 == "zero" else start)


# ---------------------------------------------------------------- the systems
SPD_DECADES, SPD_SEED = 0.5, 2
# (kind, grid, clean solve) of the preconditioned CG solver whose plain-numpy restatement its own two CPU roundings do not carry to
# 1e-12: a hierarchy that is odd at every level (33 -> 17 -> 9 -> 5; 17 -> 9 -> 5 in 3-D), run far past convergence (the account is in
# multigrid_restatement.TABLE's comment). tests/test_leftovers_host.py runs both roundings of every clean solve and asserts that a
# pair is listed here if and only if it misses the rule. Such a solve is held to the carried ones instead: a capped solve's history
# is the beginning of a longer one's, bit for bit. The 130 grid's hierarchy (130 -> 65 -> ...) is carried in every clean solve.
PCG_NOT_CARRIED = {("multigrid1", 33, "long-x0zero"), ("multigrid1", 33, "long-x0nonzero"), ("multigrid3d", 17, "long-x0zero"),
                   ("multigrid3d", 17, "long-x0nonzero"), ("multigrid3d", 17, "converging-x0nonzero")}


@functools.lru_cache(maxsize=None)
def spd(n):
    """pcg_restatement.scaled_stencil5: S A S, s_i = 10^U(0, 0.5) -- symmetric definite, a diagonal that varies over a decade."""
    import pcg_restatement as PR

    return PR.scaled_stencil5(n, SPD_DECADES, SPD_SEED)


@functools.lru_cache(maxsize=None)
def spd3(n):
    """The 3-D Poisson stencil (centre 6, neighbours -1) of multigrid3d_restatement."""
    import multigrid3d_restatement as M3

    return M3.poisson(n)


@functools.lru_cache(maxsize=None)
def upwind(n, dim=2):
    """The upwind convection-diffusion matrices of the BiCGSTAB / GCR tables (bicgstab_restatement.convdiff5 / convdiff7)."""
    import bicgstab_restatement as BR

    return BR.convdiff5(n) if dim == 2 else BR.convdiff7(n)


@functools.lru_cache(maxsize=None)
def eigenvector(symmetric, n, jacobi):
    """A right-hand side that every Krylov loop of the library is done with after one iteration: an eigenvector r0 of A M^-1, for
    M = I (jacobi False) or M = D and every polynomial in D^-1 A (jacobi True: r0 = D^1/2 u, u an eigenvector of D^-1/2 A D^-1/2;
    on the upwind matrices D is constant, so it is A's own). A middle eigenvalue, by a dense decomposition of the 2-D n x n system."""
    A = (spd(n) if symmetric else upwind(n)).toarray()
    if symmetric:
        s = np.sqrt(np.diag(A)) if jacobi else np.ones(len(A))
        _, vectors_ = np.linalg.eigh(A / np.outer(s, s))
        v = s * vectors_[:, len(A) // 2]
    else:
        values, vectors_ = np.linalg.eig(A)
        real = np.flatnonzero(np.abs(values.imag) < 1e-12 * np.abs(values.real))
        pick = real[np.argsort(values.real[real])[len(real) // 2]]
        v = vectors_[:, pick].real
    return v / np.max(np.abs(v))


MIXED_TOL, MIXED_CAP = 1e-8, 12


def mixed_batch(k, n, symmetric, jacobi):
    """The dirtying batch `mixed` of the batched solvers (one tolerance, one cap: 1e-8, 12 iterations): nan_b in slot 0, zero_b in
    slot 1, huge_long's right-hand side in slot k - 2 (no ordinary column of the table converges in 12 iterations without a
    multigrid cycle: it is capped; at k = 3 it takes slot 1 from the zero column), an early-converging column (eigenvector) in slot
    k - 1, ordinary columns between. Returns B, X0."""
    by = {d.name: d for d in DIRTY}
    cols = [vectors(Solve("normal", "normal", "nonzero", MIXED_TOL, MIXED_CAP), n, 2, seed=40 + j) for j in range(k)]
    cols[0], cols[1] = vectors(by["nan_b"], n, 2, seed=40), vectors(by["zero_b"], n, 2, seed=41)
    cols[k - 2] = vectors(by["huge_long"], n, 2, seed=42)
    cols[k - 1] = (eigenvector(symmetric, n, jacobi).copy(), np.zeros(n * n))
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols])


def column_of(x, history, stats):
    """One column from what the binding's solve wrappers return: x, the history, the statistics structure."""
    return Column(np.array(x, dtype=np.float64), np.array(history, dtype=np.float64), int(stats.iterations), int(stats.converged),
                  getattr(stats, "breakdown", None), float(stats.residual_norm))


def differences(again, fresh):
    """What differs between two results (lists of Column), bit for bit; the timing fields are not part of a Column. [] = nothing."""
    out = []
    if len(again) != len(fresh):
        return [("columns", len(again), len(fresh))]
    for j, (a, f) in enumerate(zip(again, fresh)):
        if (a.iterations, a.converged, a.breakdown) != (f.iterations, f.converged, f.breakdown):
            out.append((j, "iterations, converged, breakdown", (a.iterations, a.converged, a.breakdown), (f.iterations, f.converged, f.breakdown)))
        if not same_bits(a.history, f.history):
            out.append((j, "history", len(a.history), len(f.history),
                        [float(v) for v in a.history[:4]], [float(v) for v in f.history[:4]]))
        if not same_bits(a.x, f.x):
            bad = np.flatnonzero(np.ascontiguousarray(a.x).view(np.uint64) != np.ascontiguousarray(f.x).view(np.uint64)) \
                if a.x.shape == f.x.shape else np.zeros(0, dtype=np.int64)
            out.append((j, "x", len(bad), "non-finite", int(np.sum(~np.isfinite(a.x))), "first at", bad[:4].tolist()))
        if not same_bits([a.residual_norm], [f.residual_norm]):
            out.append((j, "residual_norm", a.residual_norm, f.residual_norm))
    return out


def reread_history(solve, fresh, label):
    """The family's *_last_history into a buffer pre-filled with SENTINEL and longer than fresh's history and than the longest of
    the table's dirtying solves: the count is fresh's, the entries are fresh's, and everything past them still holds the sentinel."""
    read = getattr(solve, "last_history", None)
    if read is None:
        return
    for j, f in enumerate(fresh):
        buf = np.full(max(HUGE_ITERS + 1, len(f.history)) + HISTORY_SLACK, SENTINEL)
        count = read(j, buf)
        assert count == len(f.history), (label, j, "history count", count, len(f.history))
        assert same_bits(buf[:count], f.history), (label, j, "history re-read differs")
        assert same_bits(buf[count:], np.full(len(buf) - count, SENTINEL)), (label, j, "written past the history's count")


def dirty_then_clean(solve, release, clean, dirty, nan_scratch=None, in_a_row=True):
    """solve(description) -> list of Column (one per right-hand side); it may carry last_history(column, buffer) -> count.
    release() drops the family's workspace (and makes a new preconditioner handle where the subject owns one). nan_scratch()
    allocates and frees a NaN-filled device vector of about the workspace's size, so that a new allocation is likely to land on NaN
    (best effort, not asserted).

    fresh = solve(clean) on the new workspace; then every dirtying solve followed by the clean solve again, and (in_a_row) all of
    them one after the other followed by it once more: each must equal fresh bit for bit in x, the whole history, iterations,
    converged, the breakdown field and the bits of residual_norm, and the family's last history must be fresh's and no longer.
    Returns fresh, for the caller to hold to the restatement: the pair cannot be equally wrong."""
    release()
    if nan_scratch is not None:
        nan_scratch()
    fresh = solve(clean)
    reread_history(solve, fresh, (clean.name, "fresh"))
    for d in dirty:
        solve(d)
        again = solve(clean)
        diff = differences(again, fresh)
        assert not diff, (clean.name, "after", d.name, diff)
        reread_history(solve, fresh, (clean.name, "after", d.name))
    if in_a_row and len(dirty) > 1:
        for d in dirty:
            solve(d)
        again = solve(clean)
        diff = differences(again, fresh)
        assert not diff, (clean.name, "after all of", [d.name for d in dirty], diff)
        reread_history(solve, fresh, (clean.name, "after all"))
    return fresh
