"""tests/leftovers.py on the CPU: the table is what it claims -- on the restatements alone, every dirtying solve ends the way its
row says and every clean solve takes the count its row says, on the matrices tests/test_leftovers_gpu.py uses --, and the harness
bites: a small fake solver with a kept ring, a kept flag record and a kept history passes, and each of its three leaky variants is
caught under the dirtying solve that was written for it."""
import numpy as np
import pytest

import bicgstab_restatement as BR
import cg_restatement as CG
import gcr_restatement as GR
import leftovers as LO
import pcg_restatement as PR
from bitwise import same_bits

GRID = 33
BY_NAME = {s.name: s for s in LO.CLEAN + LO.DIRTY}


def spd():
    return LO.spd(GRID)


def upwind():
    return LO.upwind(GRID)


def run(family, A, solve, kind="none", restart=4, O=None):
    """x, history, iterations, converged of one described solve through a family's plain restatement."""
    b, x0 = LO.vectors(solve, GRID)
    dinv = 1.0 / PR.diagonal(A) if kind == "jacobi" else None
    with np.errstate(all="ignore"):
        if family == "pcg":
            return PR.pcg(A, b, x0, dinv, solve.tol, solve.max_iters)
        if family == "bicgstab":
            return BR.bicgstab(A, b, x0, dinv, solve.tol, solve.max_iters)[:4]
        if family == "gcr":
            return GR.gcr(A, b, x0, GR.make_apply(A, 2, kind), restart, solve.tol, solve.max_iters)[:4]
        assert family == "cg"
        rp, ci, va = O.build_csr(PR.entries_of(A), A.shape[0])
        return CG.solve(CG.whole_grid(O, rp, ci, va, GRID, "row-direct", device_form=True), b, x0, solve.max_iters, solve.tol)


BREAKING = [("pcg", "none", 0), ("pcg", "jacobi", 0), ("bicgstab", "none", 0), ("bicgstab", "jacobi", 0), ("gcr", "none", 4),
            ("gcr", "jacobi", 16), ("gcr", "multigrid1", 4), ("gcr", "chebyshev2", 16)]


def matrix_of(family):
    return spd() if family in ("pcg", "cg") else upwind()


@pytest.mark.parametrize("family,kind,restart", BREAKING, ids=[f"{f}-{k}-m{m}" for f, k, m in BREAKING])
def test_the_dirtying_solves_end_as_the_table_says(family, kind, restart):
    A = matrix_of(family)
    for name in ("nan_b", "inf_b"):
        x, h, it, conv = run(family, A, BY_NAME[name], kind, restart)
        assert it == 1 and not conv and len(h) == 2 and not np.any(np.isfinite(h)), (name, it, conv, h)
    # b = 0 from x0 = 0: the first scalar of the family (p.Ap, sigma, gamma) is 0 -- a breakdown in iteration 1, never "converged"
    x, h, it, conv = run(family, A, BY_NAME["zero_b"], kind, restart)
    assert it == 1 and not conv and same_bits(h, np.zeros(2)) and same_bits(x, np.zeros(len(x))), (it, conv, h)
    x, h, it, conv = run(family, A, BY_NAME["no_iterations"], kind, restart)
    assert it == 0 and not conv and len(h) == 1 and same_bits(x, LO.vectors(BY_NAME["no_iterations"], GRID)[1])
    x, h, it, conv = run(family, A, BY_NAME["huge_long"], kind, restart)
    assert it == LO.HUGE_ITERS and not conv and len(h) == it + 1 and np.all(np.isfinite(h)) and np.all(np.isfinite(x)), (it, conv)
    assert h[0] > 1e90  # another magnitude than any clean solve's
    x, h, it, conv = run(family, A, BY_NAME["early_stop"], kind, restart)
    assert conv and 1 <= it < run(family, A, BY_NAME["converging-x0nonzero"], kind, restart)[2] and np.all(np.isfinite(h)), (it, conv)


@pytest.mark.parametrize("family,kind,restart", BREAKING, ids=[f"{f}-{k}-m{m}" for f, k, m in BREAKING])
def test_the_clean_solves_take_the_counts_of_the_table(family, kind, restart):
    A = matrix_of(family)
    for solve in LO.CLEAN:
        x, h, it, conv = run(family, A, solve, kind, restart)
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(x)) and len(h) == it + 1, solve.name
        if solve.name.startswith("short"):
            assert (it, conv) == (LO.SHORT, False), (solve.name, it, conv)
        elif solve.name.startswith("long"):
            assert (it, conv) == (LO.LONG, False), (solve.name, it, conv)
        else:
            assert conv and LO.SHORT < it < solve.max_iters, (solve.name, it, conv)


def test_plain_cg_has_no_breakdown_rule(O):
    """cg_solve_device's loop: nan_b runs all 20 iterations, past a 16-slot ring, and so does zero_b (0 / 0 is no ratio below the
    tolerance); the clean solves take the table's counts."""
    A = spd()
    for name in ("nan_b", "inf_b", "zero_b"):
        x, h, it, conv = run("cg", A, BY_NAME[name], O=O)
        assert it == LO.NAN_ITERS > LO.RING and conv == 0 and len(h) == it + 1 and not np.any(np.isfinite(h[1:])), (name, it, conv)
    x, h, it, conv = run("cg", A, BY_NAME["huge_long"], O=O)
    assert it == LO.HUGE_ITERS and conv == 0 and np.all(np.isfinite(h)) and np.all(np.isfinite(x)) and h[0] > 1e90
    x, h, it, conv = run("cg", A, BY_NAME["early_stop"], O=O)
    assert conv == 1 and 1 <= it < run("cg", A, BY_NAME["converging-x0nonzero"], O=O)[2]
    for solve in LO.CLEAN:
        x, h, it, conv = run("cg", A, solve, O=O)
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(x))
        want = {"short": (LO.SHORT, 0), "long": (LO.LONG, 0)}.get(solve.name.split("-")[0])
        assert (it, conv) == want if want else (conv == 1 and LO.SHORT < it < solve.max_iters), (solve.name, it, conv)


def test_the_inputs_of_the_table():
    for grid, dim in ((33, 2), (130, 2), (17, 3)):
        at = LO.inf_rows(grid, dim)
        assert len(set(at.tolist())) == len(at) and at.max() < grid ** dim and {int(r) // grid for r in at} == {1, grid // 2}
        b, x0 = LO.vectors(BY_NAME["inf_b"], grid, dim)
        assert np.all(np.isposinf(b[at])) and int(np.sum(~np.isfinite(b))) == len(at) and np.all(x0 != 0.0)
        b, x0 = LO.vectors(BY_NAME["nan_b"], grid, dim)
        assert np.all(np.isnan(b))
        b2, _ = LO.vectors(LO.CLEAN[0], grid, dim)
        b3, x3 = LO.vectors(LO.CLEAN[3], grid, dim)
        assert same_bits(b2, b3) and np.all(x3 != 0.0) and LO.CLEAN[0].x0 == "zero" and LO.CLEAN[3].x0 == "nonzero"
    assert len(LO.CLEAN) == 6 and [d.name for d in LO.DIRTY] == ["nan_b", "inf_b", "zero_b", "no_iterations", "huge_long", "early_stop"]
    assert [d.variant for d in LO.dirties("a", "b")[-2:]] == ["a", "b"]


# ---------------------------------------------------------------- the harness bites
class Fake:
    """A Richardson loop x += 0.25 r on A = 2 I that keeps state the way the solvers do: the steps wait in a ring of SLOTS vectors with
    an alpha slot each and are summed into x at the end (only the slots this solve filled count), a flag record with `stop`, and a
    history buffer that only grows. release() drops it all. leak: "ring" sums every slot, the unused ones with alpha 0; "stop" does not
    clear the flag; "history" hands out the kept buffer past the last solve's count."""
    SLOTS = 4

    def __init__(self, n, leak=None):
        self.n, self.leak = n, leak
        self.release()

    def release(self):
        self.ring = np.zeros((self.SLOTS, self.n))
        self.alpha = np.zeros(self.SLOTS)
        self.flags = {"stop": 0}
        self.kept = np.zeros(0)
        self.count = 0

    def __call__(self, solve):
        b, x0 = LO.vectors(solve, GRID)
        b, x0 = b[:self.n], x0[:self.n]
        if self.leak != "stop":
            self.flags["stop"] = 0
        used = np.zeros(self.SLOTS, dtype=bool)
        x, r = x0.copy(), b - 2.0 * x0
        with np.errstate(all="ignore"):
            b_norm = float(np.sqrt(r @ r))
            hist, it, converged = [b_norm], 0, 0
            if b_norm == 0.0:
                self.flags["stop"] = 1
            while it < solve.max_iters and not self.flags["stop"]:
                slot = it % self.SLOTS
                if used[slot]:  # the slot comes round again: its step goes into x first
                    x = x + self.alpha[slot] * self.ring[slot]
                self.ring[slot], self.alpha[slot], used[slot] = r, 0.25, True
                r = r - 2.0 * 0.25 * r
                it += 1
                hist.append(float(np.sqrt(r @ r)))
                if hist[-1] / b_norm < solve.tol:
                    converged = 1
                    break
            for slot in range(self.SLOTS):
                if used[slot]:
                    x = x + self.alpha[slot] * self.ring[slot]
                elif self.leak == "ring":
                    x = x + 0.0 * self.ring[slot]
        if len(hist) > len(self.kept):
            self.kept = np.concatenate([self.kept, np.zeros(len(hist) - len(self.kept))])
        self.kept[:len(hist)] = hist
        self.count = len(hist)
        return [LO.Column(x, np.array(hist), it, converged, None, hist[-1])]

    def last_history(self, column, buf):
        upto = len(self.kept) if self.leak == "history" else self.count
        buf[:min(upto, len(buf))] = self.kept[:min(upto, len(buf))]
        return self.count


def test_the_sound_fake_passes():
    fake = Fake(40)
    for clean in LO.CLEAN:
        fresh = LO.dirty_then_clean(fake, fake.release, clean, LO.DIRTY)
        assert np.all(np.isfinite(fresh[0].x)) and fresh[0].iterations >= LO.SHORT


@pytest.mark.parametrize("leak,culprit", [("ring", "nan_b"), ("stop", "zero_b"), ("history", "huge_long")])
def test_each_leaky_fake_is_caught_by_its_row(leak, culprit):
    """Caught under the dirtying solve written for it on the short clean solve (3 iterations: one ring slot stays unused), and the
    rows that do not set what it leaks let it through: the catch is the row's."""
    clean = LO.CLEAN[0]
    fake = Fake(40, leak)
    with pytest.raises(AssertionError) as err:
        LO.dirty_then_clean(fake, fake.release, clean, [BY_NAME[culprit]])
    assert culprit in str(err.value) and clean.name in str(err.value)
    LO.dirty_then_clean(fake, fake.release, clean, [BY_NAME["no_iterations"]])
    with pytest.raises(AssertionError):
        LO.dirty_then_clean(fake, fake.release, clean, LO.DIRTY)


# ---------------------------------------------------------------- what the preconditioned solves can be held to, and the mixed batch
def _pcg_roundings(kind, grid, dim, clean):
    """One clean solve of the preconditioned CG solver in plain numpy and in the other rounding."""
    import chebyshev_restatement as CH
    import multigrid3d_restatement as M3
    import multigrid_restatement as MG

    A = LO.spd(grid) if dim == 2 else LO.spd3(grid)
    b, x0 = LO.vectors(clean, grid, dim)
    dinv = 1.0 / PR.diagonal(A)
    if kind in ("none", "jacobi"):
        d = dinv if kind == "jacobi" else None
        return PR.pcg(A, b, x0, d, clean.tol, clean.max_iters), PR.pcg_other_rounding(A, b, x0, d, clean.tol, clean.max_iters)
    if kind.startswith("chebyshev"):
        lo, hi = CH.interval(A, dinv, 0.0, 0.0)
        k = int(kind[len("chebyshev"):])
        return CH.pcg(A, b, x0, k, lo, hi, clean.tol, clean.max_iters), CH.pcg_other_rounding(A, b, x0, k, lo, hi, clean.tol, clean.max_iters)
    M = MG if dim == 2 else M3
    return M.pcg(A, grid, b, x0, 1, clean.tol, clean.max_iters), M.pcg_other_rounding(A, grid, b, x0, 1, clean.tol, clean.max_iters)


PCG_KINDS = [("none", 33, 2), ("jacobi", 33, 2), ("chebyshev2", 33, 2), ("chebyshev4", 33, 2), ("multigrid1", 33, 2), ("jacobi", 130, 2),
             ("chebyshev2", 130, 2), ("multigrid1", 130, 2), ("multigrid3d", 17, 3)]


@pytest.mark.parametrize("kind,grid,dim", PCG_KINDS, ids=[f"{k}-{g}" for k, g, _ in PCG_KINDS])
def test_the_preconditioned_clean_solves_carry_a_comparison_at_1e_10(kind, grid, dim):
    """The GPU test holds a fresh preconditioned solve to the plain-numpy restatement at 1e-10, as the solver's own tests do. That
    means something only where the restatement's two CPU roundings agree far below it: equal counts, histories 1e-12 apart at the
    most (the rule of multigrid_restatement.TABLE). Every clean solve is run both ways: a (kind, grid, clean solve) is listed in
    leftovers.PCG_NOT_CARRIED if and only if it misses the rule."""
    for clean in LO.CLEAN:
        a, c = _pcg_roundings(kind, grid, dim, clean)
        assert a[2] == c[2] and a[3] == c[3] and len(a[1]) == len(c[1]), (kind, clean.name, a[2], c[2])
        err = PR.hist_err(a[1], c[1])
        print(f"{kind} {grid} {clean.name}: {a[2]} iterations, the two roundings {err:.1e} apart")
        if (kind, grid, clean.name) in LO.PCG_NOT_CARRIED:
            assert err > 1e-12, (kind, grid, clean.name, err, "listed, but the two roundings do carry it")
            continue
        assert err <= 1e-12 and np.max(np.abs(a[0] - c[0])) <= 1e-12 * np.max(np.abs(a[0])), (kind, grid, clean.name, err)


MIXED = [("pcg", "none"), ("pcg", "jacobi"), ("pcg", "chebyshev2"), ("bicgstab", "none"), ("bicgstab", "jacobi"), ("gcr", "none"),
         ("gcr", "jacobi"), ("gcr", "chebyshev2")]


@pytest.mark.parametrize("family,kind", MIXED, ids=[f"{f}-{k}" for f, k in MIXED])
def test_the_mixed_batch_is_what_it_claims(family, kind):
    """Column by column through the plain restatements: slots 0 and 1 break down in iteration 1 (at k = 3 slot 1 is slot k - 2: the
    zero column gives way), slot k - 2 is huge and still running at the cap, slot k - 1 converges within two iterations, and the ordinary columns between run to the cap."""
    import chebyshev_restatement as CH

    symmetric = family == "pcg"
    A = spd() if symmetric else upwind()
    dinv = 1.0 / PR.diagonal(A)
    for k in (3, 8):
        Bk, X0 = LO.mixed_batch(k, GRID, symmetric, kind != "none")
        ends = []
        for j in range(k):
            with np.errstate(all="ignore"):
                if family == "pcg" and kind.startswith("chebyshev"):
                    lo, hi = CH.interval(A, dinv, 0.0, 0.0)
                    out = CH.pcg(A, Bk[j], X0[j], 2, lo, hi, LO.MIXED_TOL, LO.MIXED_CAP)
                elif family == "pcg":
                    out = PR.pcg(A, Bk[j], X0[j], dinv if kind == "jacobi" else None, LO.MIXED_TOL, LO.MIXED_CAP)
                elif family == "bicgstab":
                    out = BR.bicgstab(A, Bk[j], X0[j], dinv if kind == "jacobi" else None, LO.MIXED_TOL, LO.MIXED_CAP)
                else:
                    out = GR.gcr(A, Bk[j], X0[j], GR.make_apply(A, 2, kind), 4, LO.MIXED_TOL, LO.MIXED_CAP)
            ends.append((out[2], bool(out[3])))
            if j == k - 2:
                assert out[1][0] > 1e90 and np.all(np.isfinite(out[1]))
        assert ends[0] == (1, False) and (k == 3 or ends[1] == (1, False)), ends  # k = 3: slot 1 is slot k - 2, the huge column
        assert ends[k - 2] == (LO.MIXED_CAP, False), ends
        assert ends[k - 1][1] and ends[k - 1][0] <= 2, ends
        assert all(e == (LO.MIXED_CAP, False) for e in ends[2:k - 2]), ends


def test_every_listed_pair_is_one_the_gpu_test_runs():
    assert {(k, g) for k, g, _ in LO.PCG_NOT_CARRIED} <= {(k, g) for k, g, _ in PCG_KINDS}


def test_the_restart_32_row_of_gcr_fills_every_basis_slot():
    """The other_kind row ("none", 32) of tests/test_leftovers_gpu.py: 40 iterations at tolerance 0 under restart 32, more than the 32
    basis slots GCR can hold, finite throughout."""
    d = LO.other_kind(("none", GR.MAX_RESTART), LO.LONG)
    x, h, it, conv = run("gcr", upwind(), d, "none", GR.MAX_RESTART)
    assert it == LO.LONG > GR.MAX_RESTART == LO.BASIS and not conv and np.all(np.isfinite(h)) and np.all(np.isfinite(x))
