"""The preconditioned solver's kernels (csrc/pcg.hip) one at a time, through the LAB build's spmv_amd_pcg_stage -- the launches
spmv_amd_pcg_solve_device makes, on caller data -- against the oracle's element-wise forms: as tests/test_blas1_gpu.py says, a
wrong-but-compensating element-wise operation would survive a whole-solve comparison at 1e-10, not these. Element-wise results
are BIT-exact; the two sums of a streaming stage, fed into the reduce stage, are held to 1e-13 of sum|terms| against math.fsum
(test_blas1_gpu.py's bound for a re-ordered fp64 sum) and must be bit-reproducible; the scalar step is read field by field on
totals that are exactly representable. Every output array lies between 16 sentinel doubles that must survive each call."""
import math

import numpy as np
import pytest

import reduction_restatement as R

pytestmark = pytest.mark.gpu

# one workgroup covers 128 elements; 131 073 is the largest n of the one-workgroup reduction (1024 partials, odd tail),
# 131 075 the first two-stage one (1025)
SIZES = [1, 2, 3, 127, 128, 129, 1000, 4097, 131_073, 131_075, 1_000_001]
KINDS = ["jacobi+", "jacobi-", "none"]
COUNTS = [1, 2, 255, 256, 257, 1024, 1025, 2813, 65_537]  # 2813: slice 11, 256 slices, the last short; 65 537: slice 257, the last of 2
GUARD = 16
SENTINEL = -6.02214076e23
SUM_TOL = 1e-13


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


class Guarded:
    """`values` on the device with GUARD sentinel doubles in front and behind (the payload stays 16-byte aligned)."""

    def __init__(self, Blab, values):
        self.B = Blab
        self.n = len(values)
        host = np.full(self.n + 2 * GUARD, SENTINEL)
        host[GUARD:GUARD + self.n] = values
        self.dev = Blab.DeviceVector.from_host(host)
        self.ptr = self.dev.ptr + 8 * GUARD
        assert self.ptr % 16 == 0

    def read(self):
        host = self.dev.to_host()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + self.n:] == SENTINEL), "written outside the array"
        return host[GUARD:GUARD + self.n].copy()

    def free(self):
        self.dev.free()


def partial_count(n):
    return max(1, ((n >> 1) + 63) // 64)


def vectors(n, kind, salt):
    """seed fixed per n (and stage); dinv = +-1 / U(0.5, 4), one sign per case: r.z is no multiple of r.r"""
    rng = np.random.default_rng(1000 * n + salt)
    v = [rng.standard_normal(n) for _ in range(4)]
    dinv = (-1.0 if kind == "jacobi-" else 1.0) / rng.uniform(0.5, 4.0, n)
    return v, dinv


def z_of(kind, dinv, r):
    return r.copy() if kind == "none" else dinv * r  # one product per element


def bits(x):
    return np.float64(x).view(np.uint64)


def reduce_stage(Blab, partials_ptr, count, which, incoming=None, tol=0.0, hist_ptr=None, hist_cap=0):
    sc = Blab.PcgScalars() if incoming is None else incoming
    a = Blab.PcgStageArgs(partials=partials_ptr, count=count, which=which, tol=tol, hist=hist_ptr, hist_cap=hist_cap)
    assert Blab.pcg_stage("reduce", None, a, sc) == 0
    return sc


def two_sums(Blab, partials_ptr, count):
    """The totals of value 0 and value 1 as step 0 leaves them: b_norm = sqrt(total 0), rz = total 1."""
    sc = reduce_stage(Blab, partials_ptr, count, 0)
    return sc.b_norm, sc.rz


def check_sums(Blab, partials, count, r, z, what):
    b_norm, rz = two_sums(Blab, partials.ptr, count)
    rr_terms, rz_terms = r * r, r * z
    rr_want, rz_want = math.fsum(rr_terms), math.fsum(rz_terms)
    rr_err, rz_err = abs(b_norm * b_norm - rr_want), abs(rz - rz_want)
    print(f"{what}: r.r err {rr_err / rr_want:.2e}, r.z err {rz_err / float(np.sum(np.abs(rz_terms))):.2e} of sum|terms|")
    assert rr_err <= SUM_TOL * rr_want, what                                  # the FIRST total is r.r (sqrt and square: 2 ulp)
    assert rz_err <= SUM_TOL * float(np.sum(np.abs(rz_terms))), what          # the SECOND is r.z
    again = two_sums(Blab, partials.ptr, count)
    assert again == (b_norm, rz), what                                         # fixed shape: the same bits
    return b_norm, rz


def kind_name(kind):
    return "none" if kind == "none" else "jacobi"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, O, n, kind):
    """r0 = b - Ap (fma(1, b, -Ap) and the oracle's fma(-1, Ap, b) round the same exact value once), z0 = dinv r0, p0 = z0 bit
    for bit, and the partials of r.r and r.z."""
    (b, Ap, _, _), dinv = vectors(n, kind, 1)
    count = partial_count(n)
    db, dA, dd = (Guarded(Blab, v) for v in (b, Ap, dinv))
    dr, dp, dpart = Guarded(Blab, np.full(n, np.nan)), Guarded(Blab, np.full(n, np.nan)), Guarded(Blab, np.full(2 * count, np.nan))
    a = Blab.PcgStageArgs(n=n, b=db.ptr, Ap=dA.ptr, dinv=None if kind == "none" else dd.ptr, r=dr.ptr, p=dp.ptr, partials=dpart.ptr)
    assert Blab.pcg_stage("init", kind_name(kind), a) == 0
    assert a.count == count
    want_r = O.axpy(-1.0, Ap, b)
    want_z = z_of(kind, dinv, want_r)
    r, p = dr.read(), dp.read()
    assert np.array_equal(r, want_r) and np.array_equal(p, want_z)
    first = dpart.read()
    assert np.all(np.isfinite(first))
    check_sums(Blab, dpart, count, want_r, want_z, f"init n={n} {kind}")
    assert Blab.pcg_stage("init", kind_name(kind), a) == 0
    assert np.array_equal(dpart.read(), first) and np.array_equal(dr.read(), r) and np.array_equal(dp.read(), p)
    assert np.array_equal(db.read(), b) and np.array_equal(dA.read(), Ap) and np.array_equal(dd.read(), dinv)  # inputs untouched
    for v in (db, dA, dd, dr, dp, dpart):
        v.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_r_stage(Blab, O, n, kind):
    """r' = fma(-alpha, Ap, r) with the partials of r'.r' and r'.z'; with skip_update set r keeps its bits and the sums are
    those of the unchanged r."""
    (r, Ap, _, _), dinv = vectors(n, kind, 2)
    alpha = float(np.random.default_rng(n).uniform(-2.0, 2.0))
    count = partial_count(n)
    dA, dd = Guarded(Blab, Ap), Guarded(Blab, dinv)
    for skip, want_r in ((0, O.axpy(-alpha, Ap, r)), (1, r)):
        dr, dpart = Guarded(Blab, r), Guarded(Blab, np.full(2 * count, np.nan))
        a = Blab.PcgStageArgs(n=n, Ap=dA.ptr, dinv=None if kind == "none" else dd.ptr, r=dr.ptr, partials=dpart.ptr)
        sc = Blab.PcgScalars(alpha=alpha, skip_update=skip, rz=np.nan, pAp=np.nan, beta=np.nan)
        assert Blab.pcg_stage("update_r", kind_name(kind), a, sc) == 0
        assert a.count == count
        assert np.array_equal(dr.read(), want_r), skip
        assert np.all(np.isfinite(dpart.read()))
        check_sums(Blab, dpart, count, want_r, z_of(kind, dinv, want_r), f"update_r n={n} {kind} skip={skip}")
        dr.free(), dpart.free()
    assert np.array_equal(dA.read(), Ap) and np.array_equal(dd.read(), dinv)
    dA.free(), dd.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xp_stage(Blab, O, n, kind):
    """x' = fma(alpha, p, x), p' = fma(beta, p, dinv r). skip_update: neither moves. converged, breakdown: x moves, p keeps its
    bits, and r and dinv are not read (they hold NaN)."""
    (r, p, x, _), dinv = vectors(n, kind, 3)
    rng = np.random.default_rng(n + 5)
    alpha, beta = float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-2.0, 2.0))
    want_x, want_p = O.axpy(alpha, p, x), O.update_p(z_of(kind, dinv, r), beta, p)
    nan = np.full(n, np.nan)
    cases = (("direction", dict(), r, dinv, want_x, want_p), ("skip_update", dict(skip_update=1), r, dinv, x, p),
             ("converged", dict(converged=1), nan, nan, want_x, p), ("breakdown", dict(breakdown=1), nan, nan, want_x, p),
             ("skip_update and breakdown", dict(skip_update=1, breakdown=1), nan, nan, x, p))
    for name, flags, r_in, dinv_in, x_out, p_out in cases:
        dr, dd, dp, dx = Guarded(Blab, r_in), Guarded(Blab, dinv_in), Guarded(Blab, p), Guarded(Blab, x)
        a = Blab.PcgStageArgs(n=n, r=dr.ptr, dinv=None if kind == "none" else dd.ptr, p=dp.ptr, x=dx.ptr)
        sc = Blab.PcgScalars(alpha=alpha, beta=beta, rz=np.nan, pAp=np.nan, **flags)
        assert Blab.pcg_stage("update_xp", kind_name(kind), a, sc) == 0
        assert np.array_equal(dx.read(), x_out), name
        assert np.array_equal(dp.read(), p_out), name
        assert np.array_equal(dr.read(), r_in, equal_nan=True) and np.array_equal(dd.read(), dinv_in, equal_nan=True), name
        for v in (dr, dd, dp, dx):
            v.free()


@pytest.mark.parametrize("count", COUNTS)
def test_reduction_alone(Blab, count):
    """Caller partials, value 1 another random array than value 0: one value (step 1 leaves the total in pAp) and two (step 0:
    b_norm = sqrt(total 0), so value 0 is non-negative there; step 2 with rz = 1 leaves total 1 in beta and rz). Every total has
    reduction_restatement.reduce_pcg's bits: one workgroup, two with a short last slice, 256 with one."""
    rng = np.random.default_rng(count)
    v0, v1, vs = rng.standard_normal(count) ** 2, rng.standard_normal(count), rng.standard_normal(count)
    one = Guarded(Blab, np.concatenate([vs, np.full(count, np.nan)]))  # what follows value 0 is not read
    got = reduce_stage(Blab, one.ptr, count, 1, Blab.PcgScalars(rz=1.0)).pAp
    err = abs(got - math.fsum(vs))
    print(f"count={count}: one value err {err / float(np.sum(np.abs(vs))):.2e} of sum|terms|")
    assert err <= SUM_TOL * float(np.sum(np.abs(vs)))
    assert bits(got) == bits(R.reduce_pcg(vs, count, 1)[0])
    assert reduce_stage(Blab, one.ptr, count, 1, Blab.PcgScalars(rz=1.0)).pAp == got
    two = Guarded(Blab, np.concatenate([v0, v1]))
    b_norm, rz = two_sums(Blab, two.ptr, count)
    e0, e1 = abs(b_norm * b_norm - math.fsum(v0)), abs(rz - math.fsum(v1))
    print(f"count={count}: two values err {e0 / math.fsum(v0):.2e}, {e1 / float(np.sum(np.abs(v1))):.2e} of sum|terms|")
    assert e0 <= SUM_TOL * math.fsum(v0) and e1 <= SUM_TOL * float(np.sum(np.abs(v1)))
    assert two_sums(Blab, two.ptr, count) == (b_norm, rz)
    t0, t1 = R.reduce_pcg(np.concatenate([v0, v1]), count, 2)
    assert bits(b_norm) == bits(np.sqrt(np.float64(t0))) and bits(rz) == bits(t1)
    sc = reduce_stage(Blab, two.ptr, count, 2, Blab.PcgScalars(rz=1.0, b_norm=1.0), tol=0.0)
    assert sc.residual == b_norm and sc.beta == rz and sc.rz == rz and sc.converged == 0 and sc.breakdown == 0
    assert np.array_equal(two.read(), np.concatenate([v0, v1]))
    one.free(), two.free()


def fields(sc):
    return {name: getattr(sc, name) for name, _ in sc._fields_}


def same(got, want):
    """two scalar records field by field, NaN equal to NaN, -0.0 not equal to 0.0"""
    return all(np.array_equal(np.float64(got[k]).view(np.uint64), np.float64(want[k]).view(np.uint64)) for k in want)


def step(Blab, v0, v1, which, incoming, tol=0.0, hist_cap=0):
    """One reduce + step over exactly representable partials; returns the outgoing record and the 8-entry history buffer."""
    v0 = np.asarray(v0, dtype=np.float64)
    part = Guarded(Blab, np.concatenate([v0, np.asarray(v1, dtype=np.float64)]) if which != 1 else v0)
    hist = Guarded(Blab, np.full(8, SENTINEL))
    sc = reduce_stage(Blab, part.ptr, len(v0), which, incoming, tol, hist.ptr, hist_cap)
    h = hist.read()
    part.free(), hist.free()
    return sc, h


def test_step_0_initial_scalars(Blab):
    for cap in (0, 1, 8):
        garbage = Blab.PcgScalars(7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7, 7, 7, 7)
        sc, h = step(Blab, [4.0, 4.0, 4.0, 4.0], [1.0, 2.0, -8.0, 0.5], 0, garbage, hist_cap=cap)
        assert same(fields(sc), dict(rz=-4.5, pAp=0.0, alpha=0.0, beta=0.0, b_norm=4.0, residual=4.0, iterations=0, converged=0,
                                     breakdown=0, skip_update=0))
        assert np.array_equal(h, [4.0 if cap else SENTINEL] + [SENTINEL] * 7)


def test_step_1_alpha_and_p_ap_breakdown(Blab):
    base = dict(rz=3.0, pAp=9.0, alpha=9.0, beta=0.25, b_norm=8.0, residual=2.0, iterations=3, converged=0, breakdown=0, skip_update=0)
    for rz, partials, p_ap in ((3.0, [1.0, 2.0, 4.0], 7.0), (3.0, [-1.0, -2.0, -4.0], -7.0), (-3.0, [7.0], 7.0), (1.0, [3.0], 3.0),
                               (-3.0, [-0.5, -0.25], -0.75)):  # a negative pAp and a negative rz are ordinary values
        sc, h = step(Blab, partials, None, 1, Blab.PcgScalars(**dict(base, rz=rz)), hist_cap=8)
        assert same(fields(sc), dict(base, rz=rz, pAp=p_ap, alpha=np.float64(rz) / np.float64(p_ap))), partials  # one IEEE division
        assert np.all(h == SENTINEL)
    for partials in ([0.0], [-0.0], [1.0, -1.0], [np.inf], [-np.inf], [np.nan], [np.inf, -np.inf], [1.0, np.nan, 2.0]):
        sc, _ = step(Blab, partials, None, 1, Blab.PcgScalars(**base))
        got = fields(sc)
        assert got["alpha"] == 0.0 and got["skip_update"] == 1 and not (got["pAp"] != 0.0 and np.isfinite(got["pAp"])), partials
        for k in ("rz", "beta", "b_norm", "residual", "iterations", "converged", "breakdown"):
            assert got[k] == base[k], (partials, k)


def test_step_2_history_verdict_and_beta(Blab):
    base = dict(rz=-3.0, pAp=9.0, alpha=0.5, beta=0.25, b_norm=8.0, residual=2.0, iterations=3, converged=0, breakdown=0, skip_update=0)
    rr, rz_new = [4.0, 4.0, 4.0, 4.0], [1.0, 2.0, -8.0, 0.5]  # ||r|| = 4, r.z' = -4.5: 4 / 8 = 0.5
    moved = dict(base, iterations=4, residual=4.0)
    # ordinary iteration, tol far away: beta = rz' / rz (one division), rz = rz'; history written while iterations < hist_cap
    for cap, written in ((8, True), (5, True), (4, False), (3, False), (0, False)):  # a capacity of exactly `iterations` writes nothing
        sc, h = step(Blab, rr, rz_new, 2, Blab.PcgScalars(**base), tol=1e-6, hist_cap=cap)
        assert same(fields(sc), dict(moved, beta=np.float64(-4.5) / np.float64(-3.0), rz=-4.5)), cap
        want_h = np.full(8, SENTINEL)
        if written:
            want_h[4] = 4.0
        assert np.array_equal(h, want_h), cap
    # the stopping test is STRICT: res / b_norm == tol goes on, the next double above tol stops (beta and rz untouched)
    sc, _ = step(Blab, rr, rz_new, 2, Blab.PcgScalars(**base), tol=0.5, hist_cap=8)
    assert same(fields(sc), dict(moved, beta=1.5, rz=-4.5))
    sc, h = step(Blab, rr, rz_new, 2, Blab.PcgScalars(**base), tol=float(np.nextafter(0.5, 1.0)), hist_cap=8)
    assert same(fields(sc), dict(moved, converged=1)) and h[4] == 4.0
    # converging with an unusable r.z': converged, no breakdown
    for bad in ([0.0, 0.0, 0.0, 0.0], [np.nan, 0.0, 0.0, 0.0], [np.inf, 0.0, 0.0, 0.0]):
        sc, _ = step(Blab, rr, bad, 2, Blab.PcgScalars(**base), tol=0.75)
        assert same(fields(sc), dict(moved, converged=1)), bad
    # r.z' zero or not finite, not converging: breakdown, beta and rz untouched
    for bad in ([0.0, 0.0, 0.0, 0.0], [1.0, -1.0, 2.0, -2.0], [np.nan, 1.0, 1.0, 1.0], [np.inf, 1.0, 1.0, 1.0], [np.inf, -np.inf, 1.0, 1.0],
                [-np.inf, 1.0, 1.0, 1.0]):
        sc, _ = step(Blab, rr, bad, 2, Blab.PcgScalars(**base), tol=1e-6)
        assert same(fields(sc), dict(moved, breakdown=1)), bad
    # this iteration's pAp broke down: breakdown whatever the residual says (here it would converge), beta and rz untouched
    for tol in (1e-6, 0.75):
        sc, h = step(Blab, rr, rz_new, 2, Blab.PcgScalars(**dict(base, skip_update=1, alpha=0.0)), tol=tol, hist_cap=8)
        assert same(fields(sc), dict(moved, skip_update=1, alpha=0.0, breakdown=1)), tol
        assert h[4] == 4.0
    # a positive rz and a negative r.z' are ordinary values too
    sc, _ = step(Blab, rr, rz_new, 2, Blab.PcgScalars(**dict(base, rz=2.0)), tol=1e-6)
    assert same(fields(sc), dict(moved, beta=-2.25, rz=-4.5))
