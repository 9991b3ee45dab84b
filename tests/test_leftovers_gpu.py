"""A solve inherits nothing from the one before it: every entry point that keeps device state -- cg_solve_device and its borrowed
workspace slab, the CG slab, PCG, BiCGSTAB, GCR(m), the four batched solvers, the preconditioner handles -- runs its clean solves
(tests/leftovers.py: 3 and 40 iterations at tolerance 0, one to 1e-8, each from x0 = 0 and from a non-zero x0) on a new workspace and
then again after every dirtying solve of the table on the SAME workspace: a right-hand side of NaN, +inf at the seam columns, b = 0,
no iteration at all, 69 iterations on 1e100-sized junk, and the same family under another kind, restart or degree -- and after all of
them in a row. The repeat must equal the first run bit for bit in x, the whole history, the count, the verdict and residual_norm, and
the family's last history must be the first run's and no longer. The first run is held to the restatement the suite already uses
for that solve, so the pair cannot be equally wrong. tests/test_leftovers_host.py holds the table and the harness.

The solver entry points take host arrays and copy them to the device themselves, so nothing the caller owns lies on the device
during a solve: that the caller's arrays keep their bits says only that the library writes through no const pointer, it is no guard
on the kernels. The device vectors a caller does own -- r and z of the handles' applications -- sit between NaN guards."""
import numpy as np
import pytest

import bicgstab_multi_restatement as BM
import bicgstab_restatement as BR
import cg_restatement as CG
import chebyshev_restatement as CH
import conftest
import csr_restatement as CR
import gcr_multi_restatement as GM
import gcr_restatement as GR
import layered
import leftovers as LO
import multi_rhs_restatement as M
import multigrid3d_restatement as M3
import multigrid_restatement as MG
import pcg_multi_multigrid3d_restatement as PMM3
import pcg_multi_multigrid_restatement as PMM
import pcg_multi_restatement as PM
import pcg_restatement as PR
import reduction_restatement as R
from bitwise import same_bits

pytestmark = pytest.mark.gpu
ROWLDS_KNOB = "SPMV_AMD_ROWLDS_MIN_GRID"
TOL = 1e-10  # of the preconditioned solver's own whole-solve tests (tests/test_pcg_gpu.py, test_chebyshev_gpu.py, test_multigrid*_gpu.py)
GUARD = 32
BY_NAME = {s.name: s for s in LO.CLEAN + LO.DIRTY}
_cache = {}


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()  # build_csr_struct reuses csr_mat when (rows, nnz) match
    yield
    B.lib().spmv_amd_cg_release_workspace()
    B.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- systems and operators
def matrix(symmetric, grid, dim):
    if symmetric:
        return LO.spd(grid) if dim == 2 else LO.spd3(grid)
    return LO.upwind(grid, dim)


def csr_of(O, symmetric, grid, dim):
    key = ("csr", symmetric, grid, dim)
    if key not in _cache:
        A = matrix(symmetric, grid, dim)
        e = PR.entries_of(A)
        _cache[key] = (e,) + tuple(O.build_csr(e, A.shape[0]))
    return _cache[key]


class Open:
    """An operator on one of the table's systems: `mode` and, where given, a forced `variant` (the CSR operator takes it at init,
    the stencil operators after it)."""

    def __init__(self, B, O, mode, symmetric, grid, dim=2, variant=None, expect=None):
        self.B, self.mode, self.grid, self.dim, self.variant = B, mode, grid, dim, variant
        self.A = matrix(symmetric, grid, dim)
        self.rows = self.A.shape[0]
        self.e, self.rp, self.ci, self.va = csr_of(O, symmetric, grid, dim)
        B.lib().spmv_amd_reset_host_matrices()
        self.m = B.HostMatrix(self.e, self.rows, self.rows, grid)
        self.op = B.Operator(mode)
        if variant is not None and mode == "cusparse-csr":
            assert self.op.select_variant(variant) == 0
        assert self.op.init(self.m) == 0, mode
        if variant is not None and mode != "cusparse-csr":
            assert self.op.select_variant(variant) == 0
        if expect is not None:
            assert self.op.variant() == expect, self.op.variant()
        if mode == "stencil5-csr":
            self.product = lambda v: O.spmv_stencil5(self.rp, self.ci, self.va, v, grid)
        else:
            self.product = lambda v: O.spmv_csr(self.rp, self.ci, self.va, v)

    def close(self):
        self.B.lib().spmv_amd_cg_release_workspace()
        self.op.free()
        if self.variant is not None:
            self.op.select_variant(None)


def nan_scratch(B, doubles):
    """A NaN-filled device vector of about the workspace's size, allocated and freed: what the allocator hands out next is likely
    to hold NaN (best effort, not asserted)."""
    def run():
        v = B.DeviceVector(doubles, np.nan)
        B.lib().spmv_amd_device_synchronize()
        v.free()
    return run


def kept(arrays):
    return [a.copy() for a in arrays]


def unchanged(arrays, before):
    return all(same_bits(a, c) for a, c in zip(arrays, before))


def check_bits(fresh, want, what):
    """One column against (x, history, iterations, converged, ...) of a restatement, bit for bit."""
    wx, wh, wit, wconv = want[:4]
    assert (fresh.iterations, fresh.converged) == (wit, int(wconv)), (what, fresh.iterations, fresh.converged, wit, wconv)
    assert len(fresh.history) == len(wh), what
    diff = np.flatnonzero(np.ascontiguousarray(fresh.history).view(np.uint64) != np.ascontiguousarray(wh).view(np.uint64))
    assert len(diff) == 0, (what, "history differs first at", int(diff[0]), float(fresh.history[diff[0]]), float(wh[diff[0]]))
    assert same_bits(fresh.x, wx), (what, int(np.sum(fresh.x != wx)))


def counts_of(clean, fresh, what):
    """The counts of the table: 3 and 40 iterations unconverged, or converged below the cap."""
    for col in fresh:
        if clean.name.startswith("converging"):
            assert col.converged == 1 and LO.SHORT < col.iterations < clean.max_iters, (what, clean.name, col.iterations, col.converged)
        else:
            assert (col.iterations, col.converged) == (clean.max_iters, 0), (what, clean.name, col.iterations, col.converged)
        assert np.all(np.isfinite(col.x)) and np.all(np.isfinite(col.history)) and len(col.history) == col.iterations + 1


def as_the_table_says(solve, rule, what):
    """solve, with every dirtying solve of the table held to its row on the device as well (tests/test_leftovers_host.py holds the
    rows on the restatements): the predecessor did end the way the clean solve is meant to survive. rule: the family has a breakdown
    rule (it stops in iteration 1 on a NaN, an inf or a zero right-hand side); plain CG has none and runs to its cap."""
    def run(d):
        cols = solve(d)
        for col in cols:
            ends = (col.iterations, col.converged)
            if d.name in ("nan_b", "inf_b"):
                assert ends == ((1, 0) if rule else (LO.NAN_ITERS, 0)) and not np.any(np.isfinite(col.history[1:])), (what, d.name, ends)
                assert np.all(np.isfinite(col.x)) == rule, (what, d.name, "x")  # a breakdown leaves x0; plain CG ends on NaN
            elif d.name == "zero_b":
                assert ends == ((1, 0) if rule else (LO.NAN_ITERS, 0)), (what, d.name, ends)
            elif d.name == "no_iterations":
                assert ends == (0, 0) and len(col.history) == 1, (what, d.name, ends)
            elif d.name == "huge_long":
                assert ends == (LO.HUGE_ITERS, 0) and np.all(np.isfinite(col.history)) and col.history[0] > 1e90, (what, d.name, ends)
            elif d.name == "early_stop":
                assert col.converged == 1 and 1 <= col.iterations < d.max_iters, (what, d.name, ends)
            elif d.name.startswith("other_kind"):
                assert ends == (d.max_iters, 0) and np.all(np.isfinite(col.history)), (what, d.name, ends)
        return cols

    if hasattr(solve, "last_history"):
        run.last_history = solve.last_history
    return run


def run_subject(solve, release, scratch, dirty, restate, what, cleans=LO.CLEAN, rule=True):
    """Every clean solve through leftovers.dirty_then_clean; its first run against restate(clean) (a list of restated columns)."""
    out = {}
    solve = as_the_table_says(solve, rule, what)
    for clean in cleans:
        fresh = LO.dirty_then_clean(solve, release, clean, dirty, scratch)
        counts_of(clean, fresh, what)
        want = restate(clean)
        if want is not None:
            for j, col in enumerate(fresh):
                check_bits(col, want[j], (what, clean.name, j))
        out[clean.name] = fresh
    return out


# ---------------------------------------------------------------- cg_solve_device
# (id, operator, forced variant, its name, grid, dimension, SPMV_AMD_ROWLDS_MIN_GRID, SPMV_AMD_P_RING)
CG_FORMS = [("stencil5-row-lds-130", "stencil5-csr", None, "stencil5/row-lds", 130, 2, "2"),
            ("stencil5-row-direct-33", "stencil5-csr", None, "stencil5/row-direct", 33, 2, None),
            ("csr-stream-33", "cusparse-csr", "stream", "csr/stream", 33, 2, None),
            ("csr-adaptive-33", "cusparse-csr", "adaptive", "csr/adaptive", 33, 2, None),
            ("ellpack-33", "ellpack", None, None, 33, 2, None),
            ("stencil7-row-direct-17", "stencil7-csr", "row-direct", "stencil7/row-direct", 17, 3, None)]
CG_CASES = [(f"{form[0]}-ring{ring}",) + form[1:] + (ring,) for form in CG_FORMS for ring in ("1", "4", "16")]


def cg_system(O, s, name):
    """The cg_restatement.System of cg_solve_device on an opened operator (device_form: p = fma(beta, p, r))."""
    if s.mode == "stencil5-csr":
        return CG.whole_grid(O, s.rp, s.ci, s.va, s.grid, name.split("/")[1], device_form=True)
    if s.mode == "cusparse-csr":
        return CR.system(O, s.rp, s.ci, s.va, s.variant)
    if s.mode == "ellpack":
        return CG.ellpack(O, s.rp, s.ci, s.va)
    assert s.mode == "stencil7-csr" and s.variant == "row-direct"
    return CG.System(spmv=lambda v: O.spmv_csr(s.rp, s.ci, s.va, v), pap=lambda p, ap: (R.rowdirect_partials(p, ap, s.grid), ()),
                     rr0=CG.stream_rr0, device_form=True)


@pytest.mark.parametrize("case", CG_CASES, ids=[c[0] for c in CG_CASES])
def test_cg_solve_device(B, O, monkeypatch, case):
    """Plain CG has no breakdown rule: nan_b, inf_b and zero_b run all 20 iterations with NaN in every vector, past a ring of 1, 4 and
    16 slots; the clean solve behind them flushes x from ring slots and alpha slots that hold those NaN wherever it did not write."""
    label, mode, variant, name, grid, dim, min_grid, ring = case
    if min_grid is not None:
        monkeypatch.setenv(ROWLDS_KNOB, min_grid)
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)  # read when the workspace is made
    s = Open(B, O, mode, True, grid, dim, variant, name)
    try:
        def solve(d):
            b, x0 = LO.vectors(d, grid, dim)
            before = kept((b, x0))
            x, h, st = B.cg_solve(s.op, s.m, b, x0, max_iters=d.max_iters, tol=d.tol, device=True)
            assert unchanged((b, x0), before), (label, d.name, "an input changed")
            return [LO.column_of(x, h, st)]

        solve.last_history = lambda j, buf: B.lib().spmv_amd_cg_last_history(buf.ctypes.data, len(buf))

        def restate(clean):
            key = ("cg", mode, variant, name, grid, dim, clean.name)
            if key not in _cache:
                _cache[key] = [CG.solve(cg_system(O, s, name), *LO.vectors(clean, grid, dim), clean.max_iters, clean.tol)]
            return _cache[key]

        run_subject(solve, B.lib().spmv_amd_cg_release_workspace, nan_scratch(B, (8 + int(ring)) * s.rows), LO.DIRTY, restate, label,
                    rule=False)
    finally:
        s.close()


# ---------------------------------------------------------------- the CG slab (LAB build), one rank
FROM_B, FROM_SLOT0, IN_PLACE, STORED = "from b", "from ring slot 0", "in place", "stored"
FUSED = "single rank: direction update inside the block SpMV"
DEFAULTS = {}
ALL_ON = {"run_ahead": 2, "fused_direction": 2, "zero_start": 1, "ap_recompute": 1, "first_recompute": 1}
# (id, matrix, ring, block rows, options). Each option at both values against the defaults on the scaled matrix (no tile of it is
# uniform: what an option asks for may not be eligible there, so the form each case took is printed and the forms an option switches
# OFF are asserted); every form at once on the anisotropic matrix, whose tiles are uniform, so that the fused and the recomputing forms
# ARE eligible and asserted; and there each form switched off alone against all-on, so that both values of an option are two forms.
SLAB_CASES = [("defaults-ring16", "scaled", "16", None, DEFAULTS), ("defaults-ring4", "scaled", "4", None, DEFAULTS)]
SLAB_CASES += [(f"{name}-{value}", "scaled", "16", None, {name: value}) for name, values in
               (("run_ahead", (1, 2)), ("no_overlap", (0, 1)), ("fused_direction", (0, 2)), ("zero_start", (0, 1)), ("ap_recompute", (0, 1)),
                ("first_recompute", (0, 1))) for value in values]
SLAB_CASES += [(f"all-on-aniso-ring{ring}-rows{rows}", "aniso", ring, rows, ALL_ON) for ring, rows in (("16", 8), ("4", 4), ("16", 4), ("4", 8))]
SLAB_CASES += [(f"all-on-aniso-but-{name}-0", "aniso", "16", 8, dict(ALL_ON, **{name: 0}))
               for name in ("fused_direction", "zero_start", "ap_recompute", "first_recompute")]
SLAB_GRID = 130
UPLOADS = ("never", "always", "after the first run")


def slab_entries(O, which):
    key = ("slab", which)
    if key not in _cache:
        e = PR.entries_of(LO.spd(SLAB_GRID)) if which == "scaled" else layered.layered_coo(O, SLAB_GRID, *layered.BACKGROUND)
        _cache[key] = (e,) + tuple(O.build_csr(e, SLAB_GRID * SLAB_GRID))
    return _cache[key]


def slab_form(slab, st, d, options, which, uploaded, label):
    """The form the last solve took, as the slab reports it; asserted wherever the case determines it."""
    shape, (would, took, eligible, launches), first = slab.loop_shape(), slab.ap_form(), slab.first_recompute_form()[1]
    form = (shape, took, eligible, first)
    what = (label, d.name, form, launches, st.iterations)
    assert shape.startswith("single rank"), what
    if options.get("fused_direction") == 0:
        assert shape != FUSED and not took, what
    if options.get("ap_recompute") == 0:
        assert not took and launches == 0, what
    if options.get("first_recompute") == 0 or d.max_iters == 0:
        assert first == STORED, what
    if which == "aniso":  # every tile between the first and the last grid row is uniform: whatever is asked for is eligible
        on = {name: options.get(name, 0) for name in ALL_ON}
        assert (shape == FUSED) == bool(on["fused_direction"]) and (eligible or not on["fused_direction"]), what
        recomputes = bool(on["fused_direction"] and on["ap_recompute"])
        assert took == recomputes and (not took or (st.iterations - 1 <= launches <= st.iterations if st.iterations else launches == 0)), what
        if recomputes and on["first_recompute"] and d.max_iters > 0:
            if uploaded:
                assert first == (FROM_SLOT0 if on["zero_start"] else IN_PLACE), what
            elif on["zero_start"]:
                assert first == FROM_B, what
    return form


@pytest.mark.parametrize("case", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_cg_slab(Blab, O, monkeypatch, case):
    """set_vectors / solve / gather on one slab; release() makes the slab again. Three lives per clean solve from x0 = 0: no solve ever
    uploads an x0 (the zero start: b serves as p0, in the dirtying solves too); every solve uploads its x0 (the zeros included);
    and the first run on a slab that never had an x0 uploaded, then dirtying solves that upload theirs -- beside a NaN and a huge b --
    and the clean solve with zeros uploaded over them: another form of iteration 0 than the first run took, the same bits. (After
    an upload set_vectors(b, NULL) keeps the uploaded x0 by its contract, so zeros have to be uploaded to start from zero again.)
    A clean solve from a non-zero x0 uploads every solve's x0. The form each solve took is asserted where the case determines it."""
    B = Blab
    label, which, ring, block_rows, options = case
    n = SLAB_GRID
    monkeypatch.setenv(ROWLDS_KNOB, "2")  # two column tiles, the last two columns wide; block rows 4 and 8 do not divide 130
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    e, rp, ci, va = slab_entries(O, which)
    state = {"slab": None, "upload": "always", "uploaded": False, "forms": set()}

    def release():
        if state["slab"] is not None:
            state["slab"].destroy()
        B.lib().spmv_amd_reset_host_matrices()
        slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
        assert slab.variant() == "stencil5/row-lds"
        if block_rows is not None:
            slab.set_block_rows(block_rows)
        for name, value in options.items():
            slab.set_option(name, value)
        state["slab"], state["uploaded"], state["first"] = slab, False, True

    def solve(d):
        slab = state["slab"]
        b, x0 = LO.vectors(d, n)
        before = kept((b, x0))
        # "after the first run": the first run starts from the library's own zeros; from then on every solve uploads its x0
        upload = state["upload"] == "always" or (state["upload"] == "after the first run" and not state["first"])
        state["first"] = False
        if not upload:
            assert not state["uploaded"]  # NULL keeps x0's contents: only a slab nothing was uploaded to starts from zero
            x0 = np.zeros(n * n)
        state["uploaded"] = state["uploaded"] or upload
        slab.set_vectors(b, x0 if upload else None)
        st = slab.solve(max_iters=d.max_iters, tol=d.tol)
        assert unchanged((b, x0), before if upload else (before[0], x0)), (label, d.name, "the binding's caller-side array changed")
        state["forms"].add((d.name,) + slab_form(slab, st, d, options, which, state["uploaded"], label))
        x = slab.gather()
        h = np.full(d.max_iters + 2, LO.SENTINEL)
        count = B.lib().spmv_amd_cg_slab_history(slab.h, h.ctypes.data, len(h))
        return [LO.column_of(x, h[:count], st)]

    solve.last_history = lambda j, buf: B.lib().spmv_amd_cg_slab_history(state["slab"].h, buf.ctypes.data, len(buf))

    def restate(clean):
        key = ("slab-restated", which, clean.name)
        if key not in _cache:
            _cache[key] = [CG.solve(CG.whole_grid(O, rp, ci, va, n, "row-lds"), *LO.vectors(clean, n), clean.max_iters, clean.tol)]
        return _cache[key]

    try:
        for clean in LO.CLEAN:
            for upload in (UPLOADS if clean.x0 == "zero" else ("always",)):
                state["upload"] = upload
                # without uploads every solve starts from zero, whatever its row says: the rows that differ by x0 alone still differ by b
                run_subject(solve, release, nan_scratch(B, (8 + int(ring)) * n * n), LO.DIRTY, restate, label, cleans=[clean], rule=False)
        print(f"{label}: forms taken (solve, loop shape, A p recomputed, eligible, iteration 0): {sorted(state['forms'])}")
    finally:
        if state["slab"] is not None:
            state["slab"].destroy()
        B.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- preconditioners
def make_precond(B, op, kind, dim=2, multi=0):
    """kind: "none", "jacobi", "chebyshev<K>", "multigrid<NU>"; multi: the columns of a block hierarchy (0: the single-vector one)."""
    name, k = GR.parse_kind(kind)
    if name == "chebyshev":
        return B.Precond.chebyshev(op, k)
    if name == "multigrid":
        if multi:
            return B.Precond.multigrid_multi(op, k, max_rhs=multi) if dim == 2 else B.Precond.multigrid3d_multi(op, k, max_rhs=multi)
        return B.Precond.multigrid(op, k) if dim == 2 else B.Precond.multigrid3d(op, k)
    return B.Precond(op, name)


class Handles:
    """The preconditioner handles of one subject, by kind: made on first use, made anew by renew()."""

    def __init__(self, B, s, multi=0):
        self.B, self.s, self.multi, self.h = B, s, multi, {}

    def __getitem__(self, kind):
        if kind not in self.h:
            self.h[kind] = make_precond(self.B, self.s.op, kind, self.s.dim, self.multi)
        return self.h[kind]

    def renew(self):
        for pc in self.h.values():
            pc.destroy()
        self.h = {}


class DeviceApply:
    """r -> z = M^-1 r through the library's own application on two device vectors of its own (k = 1 of the block application for a
    block hierarchy: a column's bits do not depend on k)."""

    def __init__(self, B, op, pc, n, multi=False):
        self.B, self.op, self.pc, self.multi = B, op, pc, multi
        self.r, self.z = B.DeviceVector(n, 0.0), B.DeviceVector(n, 0.0)

    def __call__(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        self.B.lib().spmv_amd_copy_to_device(self.r.ptr, r.ctypes.data, r.nbytes)
        if self.multi:
            self.pc.apply_device_multi(self.op, 1, self.r.ptr, self.z.ptr)
        else:
            self.pc.apply_device(self.op, self.r.ptr, self.z.ptr)
        return self.z.to_host()

    def free(self):
        self.r.free(), self.z.free()


def application(B, s, pc, kind, multi=False):
    """(apply, owner to free or None): "none" and "jacobi" are the statement itself, the others the library's own application, which
    test_preconditioner_handles below and the preconditioners' own tests hold to the restatement bit for bit."""
    name, _ = GR.parse_kind(kind)
    if name == "none":
        return (lambda r: r), None
    if name == "jacobi":
        dinv = 1.0 / PR.diagonal(s.A)
        return (lambda r: dinv * r), None
    a = DeviceApply(B, s.op, pc, s.rows, multi)
    return a, a


# ---------------------------------------------------------------- pcg_solve_device
# (id, operator, grid, dimension, SPMV_AMD_ROWLDS_MIN_GRID, kind, the kinds of its other_kind rows)
PCG_KINDS_2D = ("none", "jacobi", "chebyshev2", "chebyshev4", "multigrid1")
PCG_CASES = [(f"33-{kind}", "stencil5-csr", 33, 2, None, kind, tuple(k for k in PCG_KINDS_2D if k != kind)) for kind in PCG_KINDS_2D]
PCG_CASES += [(f"130-row-lds-{kind}", "stencil5-csr", 130, 2, "2", kind, others) for kind, others in
              (("jacobi", ("chebyshev2",)), ("chebyshev2", ("multigrid1", "none")), ("multigrid1", ("chebyshev2", "jacobi")))]
PCG_CASES += [("17-multigrid3d", "stencil7-csr", 17, 3, None, "multigrid1", ("chebyshev2", "none", "jacobi"))]


def pcg_restated(s, pc, kind, clean):
    """The plain-numpy restatement the preconditioned solver's own tests use, on the library's reported interval / bounds."""
    b, x0 = LO.vectors(clean, s.grid, s.dim)
    name, k = GR.parse_kind(kind)
    if name in ("none", "jacobi"):
        return PR.pcg(s.A, b, x0, 1.0 / PR.diagonal(s.A) if name == "jacobi" else None, clean.tol, clean.max_iters)
    if name == "chebyshev":
        _, lo, hi, _ = pc.chebyshev_info()
        return CH.pcg(s.A, b, x0, k, lo, hi, clean.tol, clean.max_iters)
    lmax = pc.multigrid_info()[2]
    return (MG if s.dim == 2 else M3).pcg(s.A, s.grid, b, x0, k, clean.tol, clean.max_iters, lambda_max=lmax)


def check_pcg(s, pc, kind, fresh, what):
    """The first runs of one kind against the restatement as the solver's own tests hold them: equal counts and verdicts, the
    history within 1e-10 (conftest.hist_err for "none" / "jacobi" as tests/test_pcg_gpu.py, the plain relative error for the others
    as tests/test_chebyshev_gpu.py and tests/test_multigrid*_gpu.py), x within 1e-10 / 1e-8. A clean solve the restatement does not
    carry (leftovers.PCG_NOT_CARRIED) is held to the carried ones: a capped solve's history is the beginning of a longer one's."""
    name, _ = GR.parse_kind(kind)
    tag = "multigrid3d" if (name == "multigrid" and s.dim == 3) else kind
    for clean in LO.CLEAN:
        col = fresh[clean.name][0]
        if (tag, s.grid, clean.name) in LO.PCG_NOT_CARRIED:
            continue
        xo, ho, ito, conv = pcg_restated(s, pc, kind, clean)
        assert (col.iterations, col.converged) == (ito, int(conv)) and len(col.history) == len(ho), (what, clean.name, col.iterations, ito)
        err = conftest.hist_err(col.history, ho) if name in ("none", "jacobi") else PR.hist_err(col.history, ho)
        x_err = np.max(np.abs(col.x - xo)) / np.max(np.abs(xo))
        print(f"{what} {clean.name}: {col.iterations} iterations, history {err:.2e}, x {x_err:.2e}")
        assert err < TOL and x_err <= (TOL if name in ("none", "jacobi") else 1e-8), (what, clean.name, err, x_err)
    for x0 in ("zero", "nonzero"):
        short, long_, conv = (fresh[f"{name_}-x0{x0}"][0] for name_ in ("short", "long", "converging"))
        assert same_bits(long_.history[:len(short.history)], short.history), (what, x0, "short is not the beginning of long")
        both = min(len(long_.history), len(conv.history))
        assert same_bits(long_.history[:both], conv.history[:both]), (what, x0, "long and converging part before either ends")


@pytest.mark.parametrize("case", PCG_CASES, ids=[c[0] for c in PCG_CASES])
def test_pcg_solve_device(B, O, monkeypatch, case):
    label, mode, grid, dim, min_grid, kind, others = case
    if min_grid is not None:
        monkeypatch.setenv(ROWLDS_KNOB, min_grid)
    s = Open(B, O, mode, True, grid, dim, expect="stencil5/row-lds" if min_grid else None)
    handles = Handles(B, s)
    try:
        def solve(d):
            b, x0 = LO.vectors(d, grid, dim)
            before = kept((b, x0))
            x, h, st = B.pcg_solve_device(s.op, s.m, handles[d.variant or kind], b, x0, max_iters=d.max_iters, tol=d.tol)
            assert unchanged((b, x0), before), (label, d.name, "an input changed")
            return [LO.column_of(x, h, st)]

        solve.last_history = lambda j, buf: B._pcg_lib().spmv_amd_pcg_last_history(buf.ctypes.data, len(buf))

        def release():
            B.lib().spmv_amd_cg_release_workspace()
            handles.renew()

        fresh = run_subject(solve, release, nan_scratch(B, 8 * s.rows), LO.dirties(*others), lambda clean: None, label)
        check_pcg(s, handles[kind], kind, fresh, label)
    finally:
        handles.renew()
        s.close()


def test_pcg_walks_through_the_kinds_on_one_workspace(B, O):
    """none -> chebyshev4 -> jacobi -> chebyshev2 -> multigrid1 -> none on one workspace and one set of handles: each kind's clean
    solves behind the previous kind's, with that kind's nan_b solve between them, equal the kind's first runs on a new workspace."""
    grid = 33
    walk = ("none", "chebyshev4", "jacobi", "chebyshev2", "multigrid1", "none")
    s = Open(B, O, "stencil5-csr", True, grid)
    handles = Handles(B, s)
    try:
        def solve(d, kind):
            x, h, st = B.pcg_solve_device(s.op, s.m, handles[kind], *LO.vectors(d, grid), max_iters=d.max_iters, tol=d.tol)
            return [LO.column_of(x, h, st)]

        first = {}
        for kind in set(walk):
            B.lib().spmv_amd_cg_release_workspace()
            handles.renew()
            first[kind] = {clean.name: solve(clean, kind) for clean in LO.CLEAN}
        B.lib().spmv_amd_cg_release_workspace()
        handles.renew()
        previous = None
        for kind in walk:
            for clean in LO.CLEAN:
                if previous is not None:
                    solve(BY_NAME["nan_b"], previous)
                    solve(LO.other_kind(previous), previous)
                diff = LO.differences(solve(clean, kind), first[kind][clean.name])
                assert not diff, (previous, "->", kind, clean.name, diff)
            previous = kind
    finally:
        handles.renew()
        s.close()


# ---------------------------------------------------------------- bicgstab_solve
BICGSTAB_CASES = [("33-none", "stencil5-csr", 33, 2, None, "none"), ("33-jacobi", "stencil5-csr", 33, 2, None, "jacobi"),
                  ("130-row-lds-jacobi", "stencil5-csr", 130, 2, "2", "jacobi"), ("17-stencil7-none", "stencil7-csr", 17, 3, None, "none")]


@pytest.mark.parametrize("case", BICGSTAB_CASES, ids=[c[0] for c in BICGSTAB_CASES])
def test_bicgstab_solve(B, O, monkeypatch, case):
    label, mode, grid, dim, min_grid, kind = case
    other = "jacobi" if kind == "none" else "none"
    if min_grid is not None:
        monkeypatch.setenv(ROWLDS_KNOB, min_grid)
    s = Open(B, O, mode, False, grid, dim, expect="stencil5/row-lds" if min_grid else None)
    handles = Handles(B, s)
    try:
        def solve(d):
            b, x0 = LO.vectors(d, grid, dim)
            before = kept((b, x0))
            x, h, st = B.bicgstab_solve(s.op, s.m, handles[d.variant or kind], b, x0, tol=d.tol, max_iters=d.max_iters)
            assert unchanged((b, x0), before), (label, d.name, "an input changed")
            return [LO.column_of(x, h, st)]

        solve.last_history = lambda j, buf: B._pcg_lib().spmv_amd_bicgstab_last_history(buf.ctypes.data, len(buf))

        def release():
            B.lib().spmv_amd_cg_release_workspace()
            handles.renew()

        def restate(clean):
            dinv = 1.0 / PR.diagonal(s.A) if kind == "jacobi" else None
            return [BR.bicgstab_exact(s.product, *LO.vectors(clean, grid, dim), dinv, clean.tol, clean.max_iters)]

        run_subject(solve, release, nan_scratch(B, 10 * s.rows), LO.dirties(other), restate, label)
    finally:
        handles.renew()
        s.close()


# ---------------------------------------------------------------- gcr_solve
GCR_OTHERS = (("none", 32), ("chebyshev2", 16), ("multigrid1", 4), ("jacobi", 1))


def gcr_other(variant):
    """An other_kind row of GCR: a restart-32 row runs 40 iterations, so that every basis slot GCR can hold receives a predecessor's
    vectors and the first eight are written a second time."""
    return LO.other_kind(variant, LO.LONG if variant[1] == GR.MAX_RESTART else LO.NAN_ITERS)


GCR_CASES = [(f"33-{kind}-m{restart}", "stencil5-csr", 33, 2, None, kind, restart)
             for kind in ("none", "jacobi", "chebyshev2", "multigrid1") for restart in (4, 16)]
GCR_CASES += [("130-row-lds-multigrid1-m4", "stencil5-csr", 130, 2, "2", "multigrid1", 4),
              ("130-row-lds-chebyshev2-m16", "stencil5-csr", 130, 2, "2", "chebyshev2", 16),
              ("17-stencil7-multigrid1-m4", "stencil7-csr", 17, 3, None, "multigrid1", 4)]


@pytest.mark.parametrize("case", GCR_CASES, ids=[c[0] for c in GCR_CASES])
def test_gcr_solve(B, O, monkeypatch, case):
    """The other_kind rows: restart 32 under "none" (every basis slot GCR can hold) before a restart-4 clean solve, "chebyshev2" before
    "none", the hierarchy before a kind that has none, restart 1."""
    label, mode, grid, dim, min_grid, kind, restart = case
    if min_grid is not None:
        monkeypatch.setenv(ROWLDS_KNOB, min_grid)
    s = Open(B, O, mode, False, grid, dim, expect="stencil5/row-lds" if min_grid else None)
    handles = Handles(B, s)
    try:
        def solve(d):
            b, x0 = LO.vectors(d, grid, dim)
            before = kept((b, x0))
            k, m = d.variant or (kind, restart)
            x, h, st = B.gcr_solve(s.op, s.m, handles[k], b, x0, restart=m, tol=d.tol, max_iters=d.max_iters)
            assert unchanged((b, x0), before), (label, d.name, "an input changed")
            return [LO.column_of(x, h, st)]

        solve.last_history = lambda j, buf: B._gcr_lib().spmv_amd_gcr_last_history(buf.ctypes.data, len(buf))

        def release():
            B.lib().spmv_amd_cg_release_workspace()
            handles.renew()

        def restate(clean):
            apply, owned = application(B, s, handles[kind], kind)
            try:
                return [GR.gcr_exact(s.product, *LO.vectors(clean, grid, dim), apply, restart, clean.tol, clean.max_iters)]
            finally:
                if owned is not None:
                    owned.free()

        others = [gcr_other(o) for o in GCR_OTHERS if o != (kind, restart)]
        run_subject(solve, release, nan_scratch(B, (4 + 2 * 32) * s.rows), LO.DIRTY + others, restate, label)
    finally:
        handles.renew()
        s.close()


# ---------------------------------------------------------------- the four batched solvers
KS = (3, 8)
BATCH_GRID = 33
# (family, kind, restart, the other_kind variants)
BATCHED = [("cg", "none", 0, ()), ("pcg", "jacobi", 0, ("chebyshev2", "none")), ("pcg", "chebyshev2", 0, ("multigrid1", "jacobi")),
           ("pcg", "multigrid1", 0, ("chebyshev2", "none")), ("bicgstab", "none", 0, ("jacobi",)), ("bicgstab", "jacobi", 0, ("none",)),
           ("gcr", "none", 4, (("chebyshev2", 16), ("none", 32))), ("gcr", "jacobi", 16, (("multigrid1", 4), ("none", 32))),
           ("gcr", "chebyshev2", 4, (("none", 32), ("multigrid1", 16))), ("gcr", "multigrid1", 16, (("chebyshev2", 4), ("jacobi", 1)))]


# (family, kind, restart, the other_kind variants, operator, grid, dimension, SPMV_AMD_ROWLDS_MIN_GRID, k): the row-lds SpMM and the 3-D
# block hierarchy, without `mixed` (its early column is an eigenvector of the 33 grid's matrices)
BATCHED_WIDE = [("pcg", "chebyshev2", 0, ("jacobi",), "stencil5-csr", 130, 2, "2", 8),
                ("pcg", "multigrid1", 0, ("chebyshev2",), "stencil5-csr", 130, 2, "2", 3),
                ("bicgstab", "jacobi", 0, ("none",), "stencil5-csr", 130, 2, "2", 8),
                ("gcr", "multigrid1", 4, (("none", 32),), "stencil5-csr", 130, 2, "2", 3),
                ("cg", "none", 0, (), "stencil7-csr", 17, 3, None, 8),
                ("pcg", "multigrid1", 0, ("chebyshev2", "none"), "stencil7-csr", 17, 3, None, 8),
                ("gcr", "multigrid1", 16, (("chebyshev2", 4),), "stencil7-csr", 17, 3, None, 3)]


def batch_of(d, k, grid, dim=2):
    cols = [LO.vectors(d, grid, dim, seed=j) for j in range(k)]
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols])


def restated_column(B, O, s, handles, family, kind, restart, clean, j):
    """Column j of a clean batch alone, by the family's per-column restatement (a column's bits depend neither on the batch it sits in
    nor on its slot): computed once per column, shared by k = 3 and k = 8."""
    key = ("batched", family, kind, restart, s.mode, s.grid, s.dim, clean.name, j)
    if key in _cache:
        return _cache[key]
    b, x0 = LO.vectors(clean, s.grid, s.dim, seed=j)
    name, nu = GR.parse_kind(kind)
    dinv = None if name == "none" else 1.0 / PR.diagonal(s.A)
    if family in ("cg", "pcg"):
        if name == "multigrid":
            out = (PMM if s.dim == 2 else PMM3).solve(s.A, s.grid, b, x0, nu, clean.tol, clean.max_iters,
                                                      lambda_max=handles[kind].multigrid_info()[2])
        else:
            coef = list(handles[kind].chebyshev_info()[3]) if name == "chebyshev" else None
            layout = M.grid(s.grid) if s.mode == "stencil5-csr" else M.flat()  # p.Ap is summed over the SpMM's own workgroups
            out = PM.solve(s.product, layout, b, x0, dinv, coef, clean.tol, clean.max_iters)
    elif family == "bicgstab":
        out = BM.solve(s.product, b, x0, dinv, clean.tol, clean.max_iters)
    else:
        apply, owned = application(B, s, handles[kind], kind, multi=True)
        try:
            out = GM.solve(s.product, b, x0, apply, restart, clean.tol, clean.max_iters)
        finally:
            if owned is not None:
                owned.free()
    _cache[key] = out
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", BATCHED, ids=[f"{c[0]}-{c[1]}-m{c[2]}" for c in BATCHED])
def test_batched_solvers(B, O, case, k):
    batched(B, O, case, k, "stencil5-csr", BATCH_GRID, 2, True)


@pytest.mark.parametrize("case", BATCHED_WIDE, ids=[f"{c[0]}-{c[1]}-m{c[2]}-{c[4]}-{c[5]}-k{c[8]}" for c in BATCHED_WIDE])
def test_batched_solvers_on_the_row_lds_and_the_3d_operator(B, O, monkeypatch, case):
    if case[7] is not None:
        monkeypatch.setenv(ROWLDS_KNOB, case[7])
    batched(B, O, case[:4], case[8], case[4], case[5], case[6], False)


def batched(B, O, case, k, mode, grid, dim, with_mixed):
    """The table per column (every column of a dirtying batch is the dirtying solve, on its own seed) and `mixed`: one dirtying batch
    of a NaN column, a zero column, a huge column capped while it runs and one that converges early, in slots 0, 1, k - 2 and k - 1,
    before a clean batch whose every column is running. Every clean column keeps the bits it has alone. Where the family reports its
    workspace's bytes they are non-zero and unchanged between the dirtying and the clean solve: the workspace was kept."""
    family, kind, restart, others = case
    symmetric = family in ("cg", "pcg")
    s = Open(B, O, mode, symmetric, grid, dim)
    handles = Handles(B, s, multi=8)
    L = {"cg": B._multi_lib, "pcg": B._pcg_lib, "bicgstab": B._bicgstab_multi_lib, "gcr": B._gcr_multi_lib}[family]()
    held = {"cg": L.spmv_amd_cg_multi_workspace_bytes, "pcg": L.spmv_amd_pcg_multi_workspace_bytes,
            "bicgstab": getattr(L, "spmv_amd_bicgstab_multi_workspace_bytes", None)}.get(family)
    seen = []
    try:
        def run(Bk, X0, variant, tol, max_iters):
            if family == "cg":
                return B.cg_solve_multi(s.op, s.m, Bk, X0, max_iters=max_iters, tol=tol)
            if family == "pcg":
                return B.pcg_solve_multi(s.op, s.m, handles[variant or kind], Bk, X0, max_iters=max_iters, tol=tol)
            if family == "bicgstab":
                return B.bicgstab_solve_multi(s.op, s.m, handles[variant or kind], Bk, X0, tol=tol, max_iters=max_iters)
            kd, m = variant or (kind, restart)
            return B.gcr_solve_multi(s.op, s.m, handles[kd], Bk, X0, restart=m, tol=tol, max_iters=max_iters)

        def solve(d):
            if d.rhs == "mixed":
                Bk, X0 = LO.mixed_batch(k, grid, symmetric, kind != "none")
            else:
                Bk, X0 = batch_of(d, k, grid, dim)
            before = kept((Bk, X0))
            X, hists, stats = run(Bk, X0, d.variant, d.tol, d.max_iters)
            assert unchanged((Bk, X0), before), (family, kind, d.name, "an input changed")
            if held is not None:
                seen.append((d in LO.CLEAN, int(held())))
            if d.rhs == "mixed":  # the batch is what the host test says it is: the columns end in different iterations
                ends = [(st.iterations, st.converged) for st in stats]
                broken = (LO.MIXED_CAP, 0) if family == "cg" else (1, 0)  # batched CG has no breakdown rule: the NaN column runs on
                assert ends[0] == broken and (k == 3 or ends[1] == broken) and ends[k - 1][1] == 1, (family, kind, ends)
                # (a multigrid cycle knows no eigenvector of the table and converges on the huge column inside the cap as well)
                assert kind.startswith("multigrid") or (ends[k - 1][0] <= 2 and ends[k - 2] == (LO.MIXED_CAP, 0)), (family, kind, ends)
            return [LO.column_of(X[j], hists[j], stats[j]) for j in range(k)]

        solve.last_history = lambda j, buf: getattr(L, f"spmv_amd_{family}_last_history_multi")(j, buf.ctypes.data, len(buf))

        def release():
            B.lib().spmv_amd_cg_release_workspace()
            handles.renew()
            del seen[:]

        def restate(clean):
            return [restated_column(B, O, s, handles, family, kind, restart, clean, j) for j in range(k)]

        mixed = LO.Solve("mixed", "mixed", "nonzero", LO.MIXED_TOL, LO.MIXED_CAP)
        for clean in LO.CLEAN:
            run_subject(solve, release, nan_scratch(B, 12 * k * s.rows), LO.DIRTY + [gcr_other(o) if family == "gcr" else LO.other_kind(o) for o in others] + ([mixed] if with_mixed else []), restate,
                        (family, kind, restart, mode, grid, k), cleans=[clean], rule=family != "cg")
            if held is not None:  # every clean solve found the bytes its dirtying predecessor left: non-zero and the same
                pairs = [(a[1], c[1]) for a, c in zip(seen, seen[1:]) if c[0] and not a[0]]
                assert pairs and all(a == c > 0 for a, c in pairs), (family, kind, k, clean.name, pairs)
    finally:
        handles.renew()
        s.close()


# ---------------------------------------------------------------- the preconditioner handles alone
class Guarded:
    """`values` on the device with GUARD NaNs in front and behind (the payload stays 16-byte aligned), as in the stage tests."""

    def __init__(self, B, values):
        self.n = len(values)
        host = np.full(self.n + 2 * GUARD, np.nan)
        host[GUARD:GUARD + self.n] = values
        self.before = host.copy()
        self.dev = B.DeviceVector.from_host(host)
        self.ptr = self.dev.ptr + 8 * GUARD
        assert self.ptr % 16 == 0

    def read(self):
        host = self.dev.to_host()
        assert same_bits(host[:GUARD], self.before[:GUARD]) and same_bits(host[GUARD + self.n:], self.before[GUARD + self.n:]), "padding written"
        return host[GUARD:GUARD + self.n].copy()

    def untouched(self):
        return same_bits(self.dev.to_host(), self.before)

    def free(self):
        self.dev.free()


def apply_guarded(B, s, pc, Rk, multi):
    """z = M^-1 r for the columns of Rk (k, rows) on guarded device vectors: one block application (multi) or one application per
    column. r keeps its bits, nothing is written outside z."""
    k = Rk.shape[0]
    out = np.empty_like(Rk)
    if multi:
        r, z = Guarded(B, np.ascontiguousarray(Rk.T).ravel()), Guarded(B, np.full(Rk.size, np.nan))  # row-interleaved: (row, j) at [row k + j]
        try:
            pc.apply_device_multi(s.op, k, r.ptr, z.ptr)
            out = z.read().reshape(-1, k).T.copy()
            assert r.untouched()
        finally:
            r.free(), z.free()
        return out
    for j in range(k):
        r, z = Guarded(B, Rk[j]), Guarded(B, np.full(Rk.shape[1], np.nan))
        try:
            pc.apply_device(s.op, r.ptr, z.ptr)
            out[j] = z.read()
            assert r.untouched()
        finally:
            r.free(), z.free()
    return out


# (id, operator, grid, dimension, kind, block columns: 0 = spmv_amd_precond_apply_device)
HANDLE_CASES = [("chebyshev2", "stencil5-csr", 33, 2, "chebyshev2", 0), ("chebyshev4-row-lds-130", "stencil5-csr", 130, 2, "chebyshev4", 0),
                ("multigrid1", "stencil5-csr", 33, 2, "multigrid1", 0), ("multigrid1-row-lds-130", "stencil5-csr", 130, 2, "multigrid1", 0),
                ("multigrid3d", "stencil7-csr", 17, 3, "multigrid1", 0)]
HANDLE_CASES += [(f"{name}-k{k}", mode, grid, dim, kind, k) for k in KS for name, mode, grid, dim, kind in
                 (("multigrid-multi", "stencil5-csr", 33, 2, "multigrid1"), ("multigrid3d-multi", "stencil7-csr", 17, 3, "multigrid1"),
                  ("block-chebyshev2", "stencil5-csr", 33, 2, "chebyshev2"))]


@pytest.mark.parametrize("case", HANDLE_CASES, ids=[c[0] for c in HANDLE_CASES])
def test_preconditioner_handles(B, O, monkeypatch, case):
    """The handle's own vectors (Chebyshev d / z; per multigrid level r, d, z, aux and the partials) after an all-NaN r, an r with
    +inf at the seam positions and 1e100 r': a clean r on the same handle gives the bits of a new handle's application, which are the
    restatement's (gcr_restatement.exact_apply on the library's reported bounds)."""
    label, mode, grid, dim, kind, k = case
    if grid == 130:
        monkeypatch.setenv(ROWLDS_KNOB, "2")
    s = Open(B, O, mode, True, grid, dim)
    cols = max(k, 1)
    rng = np.random.default_rng(500 + grid + cols)
    clean = rng.standard_normal((cols, s.rows))
    nan = np.full((cols, s.rows), np.nan)
    inf = rng.standard_normal((cols, s.rows))
    inf[:, LO.inf_rows(grid, dim)] = np.inf
    huge = 1e100 * rng.standard_normal((cols, s.rows))
    new = make_precond(B, s.op, kind, dim, multi=k)
    used = make_precond(B, s.op, kind, dim, multi=k)
    try:
        want = apply_guarded(B, s, new, clean, bool(k))
        lmax = new.chebyshev_info()[2] if kind.startswith("chebyshev") else new.multigrid_info()[2]
        exact = GR.exact_apply(O, s.A, dim, kind, lambda_max=lmax)
        for j in range(cols):
            assert same_bits(want[j], exact(clean[j])), (label, j, "a new handle's application is not the restatement's")
        for name, dirty in (("nan", nan), ("inf", inf), ("huge", huge), ("all three", None)):
            for d in ([nan, inf, huge] if dirty is None else [dirty]):
                with np.errstate(all="ignore"):
                    apply_guarded(B, s, used, d, bool(k))
            got = apply_guarded(B, s, used, clean, bool(k))
            for j in range(cols):
                assert same_bits(got[j], want[j]), (label, "after", name, j, int(np.sum(~np.isfinite(got[j]))))
    finally:
        new.destroy(), used.destroy()
        s.close()


def test_a_handle_passes_from_a_nan_solve_to_another_family(B, O):
    """One handle per kind: PCG's nan_b solve, then GCR's clean solves through the same handle; batched PCG's NaN batch, then batched
    GCR's clean batch through the same block handle. Each equals the solve through a handle nothing has used."""
    grid, k = 33, 3
    for kind in ("chebyshev2", "multigrid1"):
        # the handle belongs to one operator, so both families solve the symmetric system (GCR takes any matrix)
        s = Open(B, O, "stencil5-csr", True, grid)
        try:
            for clean in LO.CLEAN:
                b, x0 = LO.vectors(clean, grid)
                new, used = make_precond(B, s.op, kind), make_precond(B, s.op, kind)
                want = B.gcr_solve(s.op, s.m, new, b, x0, restart=4, tol=clean.tol, max_iters=clean.max_iters)
                B.pcg_solve_device(s.op, s.m, used, *LO.vectors(BY_NAME["nan_b"], grid), max_iters=LO.NAN_ITERS, tol=0.0)
                B.pcg_solve_device(s.op, s.m, used, *LO.vectors(BY_NAME["huge_long"], grid), max_iters=LO.HUGE_ITERS, tol=0.0)
                got = B.gcr_solve(s.op, s.m, used, b, x0, restart=4, tol=clean.tol, max_iters=clean.max_iters)
                diff = LO.differences([LO.column_of(*got)], [LO.column_of(*want)])
                assert not diff, (kind, clean.name, diff)
                new.destroy(), used.destroy()
                Bk, X0 = batch_of(clean, k, grid)
                new, used = make_precond(B, s.op, kind, 2, multi=k), make_precond(B, s.op, kind, 2, multi=k)
                want = B.gcr_solve_multi(s.op, s.m, new, Bk, X0, restart=4, tol=clean.tol, max_iters=clean.max_iters)
                B.pcg_solve_multi(s.op, s.m, used, *batch_of(BY_NAME["nan_b"], k, grid), max_iters=LO.NAN_ITERS, tol=0.0)
                B.pcg_solve_multi(s.op, s.m, used, *LO.mixed_batch(k, grid, True, True), max_iters=LO.MIXED_CAP, tol=LO.MIXED_TOL)
                got = B.gcr_solve_multi(s.op, s.m, used, Bk, X0, restart=4, tol=clean.tol, max_iters=clean.max_iters)
                diff = LO.differences([LO.column_of(got[0][j], got[1][j], got[2][j]) for j in range(k)],
                                      [LO.column_of(want[0][j], want[1][j], want[2][j]) for j in range(k)])
                assert not diff, (kind, "batched", clean.name, diff)
                new.destroy(), used.destroy()
        finally:
            s.close()


# ---------------------------------------------------------------- across families
def test_across_families_on_one_operator(B, O):
    """One operator (the symmetric 33 grid: every family takes it), one set of handles. Every family's first runs on a new workspace;
    then every family runs its dirtying solves in turn; then every family's clean solves in a seeded shuffled order, twice, equal its
    first runs."""
    grid, k = 33, 3
    s = Open(B, O, "stencil5-csr", True, grid)
    single, block = Handles(B, s), Handles(B, s, multi=k)
    try:
        def one(fn):
            return lambda d: [LO.column_of(*fn(d, *LO.vectors(d, grid)))]

        def many(fn):
            def run(d):
                Bk, X0 = LO.mixed_batch(k, grid, True, True) if d.rhs == "mixed" else batch_of(d, k, grid)
                X, hists, stats = fn(d, Bk, X0)
                return [LO.column_of(X[j], hists[j], stats[j]) for j in range(k)]
            return run

        cap = lambda d: dict(tol=d.tol, max_iters=d.max_iters)  # noqa: E731
        families = {
            "cg": one(lambda d, b, x0: B.cg_solve(s.op, s.m, b, x0, device=True, **cap(d))),
            "pcg-chebyshev2": one(lambda d, b, x0: B.pcg_solve_device(s.op, s.m, single["chebyshev2"], b, x0, **cap(d))),
            "pcg-multigrid1": one(lambda d, b, x0: B.pcg_solve_device(s.op, s.m, single["multigrid1"], b, x0, **cap(d))),
            "bicgstab-jacobi": one(lambda d, b, x0: B.bicgstab_solve(s.op, s.m, single["jacobi"], b, x0, **cap(d))),
            "gcr-multigrid1-m4": one(lambda d, b, x0: B.gcr_solve(s.op, s.m, single["multigrid1"], b, x0, restart=4, **cap(d))),
            "gcr-chebyshev2-m16": one(lambda d, b, x0: B.gcr_solve(s.op, s.m, single["chebyshev2"], b, x0, restart=16, **cap(d))),
            "cg-multi": many(lambda d, Bk, X0: B.cg_solve_multi(s.op, s.m, Bk, X0, **cap(d))),
            "pcg-multi-multigrid1": many(lambda d, Bk, X0: B.pcg_solve_multi(s.op, s.m, block["multigrid1"], Bk, X0, **cap(d))),
            "bicgstab-multi-jacobi": many(lambda d, Bk, X0: B.bicgstab_solve_multi(s.op, s.m, block["jacobi"], Bk, X0, **cap(d))),
            "gcr-multi-chebyshev2-m4": many(lambda d, Bk, X0: B.gcr_solve_multi(s.op, s.m, block["chebyshev2"], Bk, X0, restart=4, **cap(d))),
        }
        first = {}
        for name, solve in families.items():
            B.lib().spmv_amd_cg_release_workspace()
            single.renew(), block.renew()
            first[name] = {clean.name: solve(clean) for clean in LO.CLEAN}
        B.lib().spmv_amd_cg_release_workspace()
        single.renew(), block.renew()
        mixed = LO.Solve("mixed", "mixed", "nonzero", LO.MIXED_TOL, LO.MIXED_CAP)
        for name, solve in families.items():
            for d in LO.DIRTY + ([mixed] if "-multi-" in name + "-" else []):
                solve(d)
        order = [(name, clean) for name in families for clean in LO.CLEAN]
        rng = np.random.default_rng(2024)
        for turn in range(2):
            for i in rng.permutation(len(order)):
                name, clean = order[i]
                diff = LO.differences(families[name](clean), first[name][clean.name])
                assert not diff, (name, clean.name, "turn", turn, diff)
    finally:
        single.renew(), block.renew()
        s.close()
