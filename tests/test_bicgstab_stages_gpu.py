"""The BiCGSTAB solver's kernels (csrc/bicgstab.hip) one at a time, through the LAB build's spmv_amd_bicgstab_stage -- the launches
spmv_amd_bicgstab_solve_device makes, on caller data -- against the restatement, BIT for bit: element-wise results against the
oracle's fma, the partials against reduction_restatement.stream_partials, the sums against reduce_pcg, the scalar step field by
field in each of its branches. Every vector lies inside a larger buffer with NaN in front and behind; the padding and the read-only
inputs must keep their bits, and a kernel launched behind a set verdict must change no bit of anything."""
import numpy as np
import pytest

import reduction_restatement as R

pytestmark = pytest.mark.gpu

# an odd tail alone, one pair, pair + tail, 63 pairs + tail, one full wave, a wave + tail, several workgroups with a tail, and
# 2 * 64 * 5 + 1: five full workgroups and the tail
SIZES = [1, 2, 3, 127, 128, 129, 4225, 2 * 64 * 5 + 1]
KINDS = ["none", "jacobi"]
COUNTS = [1, 1024, 1025, 70_000]  # one workgroup, its largest, the first two-stage one, slice 274 in 256 slices with the last short
GUARD = 16
NAMES = ("b", "dinv", "x", "r", "rhat", "p", "phat", "shat", "v", "t")


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == np.shape(b) and np.array_equal(bits(a), bits(b))


class Guarded:
    """`values` on the device with GUARD NaNs in front and behind (the payload stays 16-byte aligned)."""

    def __init__(self, Blab, values):
        self.n = len(values)
        host = np.full(self.n + 2 * GUARD, np.nan)
        host[GUARD:GUARD + self.n] = values
        self.before = host.copy()
        self.dev = Blab.DeviceVector.from_host(host)
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


class Stage:
    """The ten vectors of a stage call from `values` (name -> array; a name left out is a null pointer) and a NaN partials buffer."""

    def __init__(self, Blab, n, kind, **values):
        self.B, self.n, self.kind = Blab, n, kind
        self.count = R.stream_count(n)
        self.g = {k: Guarded(Blab, v) for k, v in values.items()}
        self.g["partials"] = Guarded(Blab, np.full(2 * self.count, np.nan))
        self.args = Blab.BicgstabStageArgs(n=n, **{k: g.ptr for k, g in self.g.items()})

    def run(self, stage, scalars=None):
        assert self.B.bicgstab_stage(stage, self.kind, self.args, scalars) == 0
        assert self.args.count == self.count
        return {k: g.read() for k, g in self.g.items()}

    def only_changed(self, *names):
        return all(g.untouched() for k, g in self.g.items() if k not in names)

    def free(self):
        for g in self.g.values():
            g.free()


def data(n, salt, names):
    rng = np.random.default_rng(1000 * n + salt)
    d = {k: rng.standard_normal(n) for k in names if k != "dinv"}
    if "dinv" in names:
        d["dinv"] = rng.choice([-1.0, 1.0]) / rng.uniform(0.5, 4.0, n)
    return d, rng


def hat(kind, dinv, u):
    return u.copy() if kind == "none" else dinv * u  # one product per element


def fma(O, a, u, c):
    return O.fma(np.full(len(u), a), u, c)


def scalars(Blab, **kw):
    base = dict(rho=np.nan, sigma=np.nan, alpha=np.nan, omega=np.nan, beta=np.nan, b_norm=np.nan, residual=np.nan, s_norm=np.nan)
    base.update(kw)
    return Blab.BicgstabScalars(**base)


def jac_only(kind, *names):
    return names if kind == "jacobi" else ()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, n, kind):
    """r = fma(1.0, b, -1.0 * v) (the difference rounded once), r^ = r, p = r, p^ = dinv p, the partials of r.r."""
    d, _ = data(n, 1, ("b", "v") + jac_only(kind, "dinv"))
    nan = np.full(n, np.nan)
    s = Stage(Blab, n, kind, r=nan, rhat=nan, p=nan, **{k: nan for k in jac_only(kind, "phat")}, **d)
    got = s.run("init")
    want = d["b"] - d["v"]
    assert same_bits(got["r"], want) and same_bits(got["rhat"], want) and same_bits(got["p"], want)
    if kind == "jacobi":
        assert same_bits(got["phat"], d["dinv"] * want)
    assert same_bits(got["partials"][:s.count], R.stream_partials(want, want)) and np.all(np.isnan(got["partials"][s.count:]))
    assert s.only_changed("r", "rhat", "p", "phat", "partials")
    s.free()


@pytest.mark.parametrize("n", SIZES)
def test_dot_rv_stage(Blab, n):
    d, _ = data(n, 2, ("rhat", "v"))
    s = Stage(Blab, n, None, **d)
    got = s.run("dot_rv")
    assert same_bits(got["partials"][:s.count], R.stream_partials(d["rhat"], d["v"])) and np.all(np.isnan(got["partials"][s.count:]))
    assert s.only_changed("partials")
    s.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_s_stage(Blab, O, n, kind):
    """s = fma(-alpha, v, r) in place, s^ = dinv s, the partials of s.s; behind a verdict nothing at all."""
    d, rng = data(n, 3, ("v", "r") + jac_only(kind, "dinv"))
    alpha = float(rng.uniform(-2.0, 2.0))
    extra = {k: np.full(n, np.nan) for k in jac_only(kind, "shat")}
    s = Stage(Blab, n, kind, **d, **extra)
    got = s.run("update_s", scalars(Blab, alpha=alpha, stop=1))
    assert s.only_changed()
    got = s.run("update_s", scalars(Blab, alpha=alpha))
    want = fma(O, -alpha, d["v"], d["r"])
    assert same_bits(got["r"], want)
    if kind == "jacobi":
        assert same_bits(got["shat"], d["dinv"] * want)
    assert same_bits(got["partials"][:s.count], R.stream_partials(want, want)) and np.all(np.isnan(got["partials"][s.count:]))
    assert s.only_changed("r", "shat", "partials")
    s.free()


@pytest.mark.parametrize("n", SIZES)
def test_dot_t_stage(Blab, n):
    """t.s (value 0) and t.t (value 1), s read from r; behind a verdict nothing at all."""
    d, _ = data(n, 4, ("t", "r"))
    s = Stage(Blab, n, None, **d)
    s.run("dot_t", scalars(Blab, stop=1))
    assert s.only_changed()
    got = s.run("dot_t", scalars(Blab))
    assert same_bits(got["partials"], np.concatenate([R.stream_partials(d["t"], d["r"]), R.stream_partials(d["t"], d["t"])]))
    assert s.only_changed("partials")
    s.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xr_stage(Blab, O, n, kind):
    """x_step 2: x = fma(omega, s^, fma(alpha, p^, x)), r = fma(-omega, t, s), the partials of r.r and r^.r. x_step 1: the half
    step, x = fma(alpha, p^, x) and nothing else. x_step 0: nothing at all."""
    jac = kind == "jacobi"
    d, rng = data(n, 5, ("x", "r", "t", "rhat") + (("phat", "shat") if jac else ("p",)))
    alpha, omega = float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-2.0, 2.0))
    ph, sh = (d["phat"], d["shat"]) if jac else (d["p"], d["r"])
    half = fma(O, alpha, ph, d["x"])
    for step, want_x in ((0, d["x"]), (1, half), (2, fma(O, omega, sh, half))):
        s = Stage(Blab, n, kind, **d)
        got = s.run("update_xr", scalars(Blab, alpha=alpha, omega=omega, x_step=step))
        assert same_bits(got["x"], want_x), step
        if step == 2:
            want_r = fma(O, -omega, d["t"], d["r"])
            assert same_bits(got["r"], want_r)
            assert same_bits(got["partials"], np.concatenate([R.stream_partials(want_r, want_r), R.stream_partials(d["rhat"], want_r)]))
            assert s.only_changed("x", "r", "partials")
        else:
            assert s.only_changed(*(("x",) if step == 1 else ())), step
        s.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_direction_stage(Blab, O, n, kind):
    """p = fma(beta, fma(-omega, v, p), r), p^ = dinv p; behind a verdict nothing at all."""
    d, rng = data(n, 6, ("p", "v", "r") + jac_only(kind, "dinv"))
    omega, beta = float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-2.0, 2.0))
    extra = {k: np.full(n, np.nan) for k in jac_only(kind, "phat")}
    s = Stage(Blab, n, kind, **d, **extra)
    assert Blab.bicgstab_stage("direction", kind, s.args, scalars(Blab, omega=omega, beta=beta, stop=1)) == 0
    assert s.only_changed()
    assert Blab.bicgstab_stage("direction", kind, s.args, scalars(Blab, omega=omega, beta=beta)) == 0
    want = fma(O, beta, fma(O, -omega, d["v"], d["p"]), d["r"])
    assert same_bits(s.g["p"].read(), want)
    if kind == "jacobi":
        assert same_bits(s.g["phat"].read(), d["dinv"] * want)
    assert s.only_changed("p", "phat")
    s.free()


# ---------------------------------------------------------------- the reducing launch
def reduce_stage(Blab, partials_ptr, count, which, incoming, tol=0.0, hist_ptr=None, hist_cap=0):
    a = Blab.BicgstabStageArgs(partials=partials_ptr, count=count, which=which, tol=tol, hist=hist_ptr, hist_cap=hist_cap)
    assert Blab.bicgstab_stage("reduce", None, a, incoming) == 0
    return incoming


@pytest.mark.parametrize("count", COUNTS)
def test_reduction_alone(Blab, count):
    """One value (step 0 leaves the total in rho, step 1 in sigma, step 2 its root in s_norm) and two (step 3: omega = total 0 / total 1; step 4 with rho = alpha = omega = 1
    leaves sqrt(total 0) in residual and total 1 in rho and beta): reduce_pcg's bits, twice the same, what follows a single value
    is not read, and a sum behind a verdict changes no field."""
    rng = np.random.default_rng(count)
    v0, v1 = rng.standard_normal(count) ** 2, rng.standard_normal(count)
    one = Guarded(Blab, np.concatenate([v0, np.full(count, np.nan)]))
    want0 = R.reduce_pcg(v0, count, 1)[0]
    for _ in range(2):
        sc = reduce_stage(Blab, one.ptr, count, 0, scalars(Blab))
        assert bits(sc.rho) == bits(want0) and bits(sc.b_norm) == bits(np.sqrt(want0))
        sc = reduce_stage(Blab, one.ptr, count, 1, scalars(Blab, rho=1.0))
        assert bits(sc.sigma) == bits(want0) and bits(sc.alpha) == bits(np.float64(1.0) / np.float64(want0)) and sc.stop == 0
        sc = reduce_stage(Blab, one.ptr, count, 2, scalars(Blab, b_norm=1.0))
        assert bits(sc.s_norm) == bits(np.sqrt(want0)) and sc.stop == 0
    two = Guarded(Blab, np.concatenate([v0, v1]))
    t0, t1 = R.reduce_pcg(np.concatenate([v0, v1]), count, 2)
    assert bits(t0) == bits(want0)
    for _ in range(2):
        sc = reduce_stage(Blab, two.ptr, count, 3, scalars(Blab))
        assert bits(sc.omega) == bits(np.float64(t0) / np.float64(t1)) and sc.stop == 0
        sc = reduce_stage(Blab, two.ptr, count, 4, scalars(Blab, rho=1.0, alpha=1.0, omega=1.0, b_norm=1.0))
        assert bits(sc.residual) == bits(np.sqrt(t0)) and bits(sc.rho) == bits(t1) and bits(sc.beta) == bits(t1) and sc.iterations == 1
    for which in (2, 3, 4):
        before = scalars(Blab, rho=3.0, alpha=0.5, omega=0.25, b_norm=1.0, s_norm=2.0, iterations=3, stop=1, x_step=1, converged=1)
        after = reduce_stage(Blab, two.ptr, count, which, scalars(Blab, rho=3.0, alpha=0.5, omega=0.25, b_norm=1.0, s_norm=2.0,
                                                                  iterations=3, stop=1, x_step=1, converged=1))
        assert same(fields(after), fields(before)), which
    assert one.untouched() and two.untouched()
    one.free(), two.free()


def fields(sc):
    return {name: getattr(sc, name) for name, _ in sc._fields_}


def same(got, want):
    """two scalar records field by field, NaN equal to NaN, -0.0 not equal to 0.0"""
    return all(np.array_equal(bits(np.float64(got[k])), bits(np.float64(want[k]))) for k in want)


def step(Blab, which, incoming, v0, v1=None, tol=0.0, hist_cap=8):
    """One reduce + step over exactly representable partials; returns the outgoing record and the 8-entry history buffer."""
    v0 = np.asarray(v0, dtype=np.float64)
    part = Guarded(Blab, v0 if v1 is None else np.concatenate([v0, np.asarray(v1, dtype=np.float64)]))
    hist = Guarded(Blab, np.full(8, -7.0))
    sc = reduce_stage(Blab, part.ptr, len(v0), which, Blab.BicgstabScalars(**incoming), tol, hist.ptr, hist_cap)
    h = hist.read()
    part.free(), hist.free()
    return fields(sc), h


BASE = dict(rho=3.0, sigma=9.0, alpha=0.5, omega=0.25, beta=0.125, b_norm=8.0, residual=2.0, s_norm=1.0, iterations=3, converged=0,
            breakdown=0, x_step=2, stop=0, pad=0)
UNUSABLE = ([0.0], [-0.0], [1.0, -1.0], [np.inf], [-np.inf], [np.nan], [np.inf, -np.inf], [1.0, np.nan, 2.0])
QUIET = np.full(8, -7.0)


def recorded(slot, value):
    h = QUIET.copy()
    h[slot] = value
    return h


def test_step_0_initial_scalars(Blab):
    garbage = dict(rho=7.0, sigma=7.0, alpha=7.0, omega=7.0, beta=7.0, b_norm=7.0, residual=7.0, s_norm=7.0, iterations=7, converged=7,
                   breakdown=7, x_step=7, stop=7, pad=7)
    for cap in (0, 1, 8):
        sc, h = step(Blab, 0, garbage, [4.0, 4.0, 4.0, 4.0], hist_cap=cap)
        assert same(sc, dict(rho=16.0, sigma=0.0, alpha=0.0, omega=0.0, beta=0.0, b_norm=4.0, residual=4.0, s_norm=0.0, iterations=0,
                             converged=0, breakdown=0, x_step=0, stop=0, pad=0))
        assert np.array_equal(h, recorded(0, 4.0) if cap else QUIET)


def test_step_1_alpha_and_the_sigma_breakdown(Blab):
    for rho, partials, sigma in ((3.0, [1.0, 2.0, 4.0], 7.0), (3.0, [-1.0, -2.0, -4.0], -7.0), (-3.0, [7.0], 7.0), (1.0, [3.0], 3.0)):
        sc, h = step(Blab, 1, dict(BASE, rho=rho, x_step=0), partials)  # a negative sigma and a negative rho are ordinary values
        assert same(sc, dict(BASE, rho=rho, sigma=sigma, alpha=np.float64(rho) / np.float64(sigma), x_step=2)), partials
        assert np.array_equal(h, QUIET)
    for partials in UNUSABLE:  # the iteration is counted, the unchanged residual recorded, nothing will be updated
        sc, h = step(Blab, 1, dict(BASE), partials)
        assert not (sc["sigma"] != 0.0 and np.isfinite(sc["sigma"])), partials
        assert same({k: v for k, v in sc.items() if k != "sigma"},
                    {k: v for k, v in dict(BASE, alpha=0.0, x_step=0, breakdown=1, stop=1, iterations=4).items() if k != "sigma"}), partials
        assert np.array_equal(h, recorded(4, 2.0)), partials
    sc, h = step(Blab, 1, dict(BASE), [0.0], hist_cap=4)  # hist_cap reached: counted, not written
    assert sc["iterations"] == 4 and sc["breakdown"] == 1 and np.array_equal(h, QUIET)


def test_step_2_the_half_step(Blab):
    ss = [4.0, 4.0, 4.0, 4.0]  # ||s|| = 4, ||r0|| = 8: 0.5
    sc, h = step(Blab, 2, dict(BASE), ss, tol=1e-6)
    assert same(sc, dict(BASE, s_norm=4.0)) and np.array_equal(h, QUIET)
    sc, h = step(Blab, 2, dict(BASE), ss, tol=0.5)  # STRICT: equal to tol goes on
    assert same(sc, dict(BASE, s_norm=4.0)) and np.array_equal(h, QUIET)
    taken = dict(BASE, s_norm=4.0, residual=4.0, iterations=4, converged=1, stop=1, x_step=1)
    for cap, written in ((8, True), (5, True), (4, False), (0, False)):
        sc, h = step(Blab, 2, dict(BASE), ss, tol=float(np.nextafter(0.5, 1.0)), hist_cap=cap)
        assert same(sc, taken) and np.array_equal(h, recorded(4, 4.0) if written else QUIET), cap
    sc, h = step(Blab, 2, dict(BASE), [np.nan], tol=1.0)  # NaN is not below anything
    assert sc["stop"] == 0 and sc["x_step"] == 2 and np.isnan(sc["s_norm"]) and np.array_equal(h, QUIET)
    sc, h = step(Blab, 2, dict(BASE), [0.0], tol=0.0)  # nor is 0 below 0
    assert same(sc, dict(BASE, s_norm=0.0)) and np.array_equal(h, QUIET)


def test_step_3_omega_and_its_breakdown(Blab):
    sc, h = step(Blab, 3, dict(BASE), [1.0, 2.0], [4.0, -10.0])  # t.s = 3, t.t = -6 (never so on real data; an ordinary value here)
    assert same(sc, dict(BASE, omega=-0.5)) and np.array_equal(h, QUIET)
    sc, _ = step(Blab, 3, dict(BASE), [1.0], [3.0])
    assert same(sc, dict(BASE, omega=np.float64(1.0) / np.float64(3.0)))
    broken = dict(BASE, omega=0.0, x_step=1, breakdown=2, stop=1, iterations=4, residual=1.0)  # ||s|| recorded, the half step's x kept
    for bad in UNUSABLE:
        for ts, tt in ((bad, [2.0] * len(bad)), ([2.0] * len(bad), bad)):
            sc, h = step(Blab, 3, dict(BASE), ts, tt)
            assert same(sc, broken) and np.array_equal(h, recorded(4, 1.0)), (ts, tt)
    sc, h = step(Blab, 3, dict(BASE), [0.0], [1.0], hist_cap=3)
    assert same(sc, broken) and np.array_equal(h, QUIET)


def test_step_4_history_verdict_and_beta(Blab):
    rr, rho_new = [4.0, 4.0, 4.0, 4.0], [1.0, 2.0, -8.0, 0.5]  # ||r|| = 4, rho' = -4.5: 4 / 8 = 0.5
    moved = dict(BASE, iterations=4, residual=4.0)
    beta = (np.float64(-4.5) / np.float64(3.0)) * (np.float64(0.5) / np.float64(0.25))
    for cap, written in ((8, True), (5, True), (4, False), (3, False), (0, False)):  # a capacity of exactly `iterations` writes nothing
        sc, h = step(Blab, 4, dict(BASE), rr, rho_new, tol=1e-6, hist_cap=cap)
        assert same(sc, dict(moved, beta=beta, rho=-4.5)), cap
        assert np.array_equal(h, recorded(4, 4.0) if written else QUIET), cap
    sc, _ = step(Blab, 4, dict(BASE, rho=7.0, alpha=3.0, omega=11.0), rr, [5.0, 0.0, 0.0, 0.0], tol=1e-6)  # (rho'/rho) * (alpha/omega)
    assert same(sc, dict(moved, alpha=3.0, omega=11.0, rho=5.0, beta=(np.float64(5.0) / np.float64(7.0)) * (np.float64(3.0) / np.float64(11.0))))
    sc, _ = step(Blab, 4, dict(BASE), rr, rho_new, tol=0.5)  # STRICT
    assert same(sc, dict(moved, beta=beta, rho=-4.5))
    sc, h = step(Blab, 4, dict(BASE), rr, rho_new, tol=float(np.nextafter(0.5, 1.0)))
    assert same(sc, dict(moved, converged=1, stop=1)) and h[4] == 4.0
    for bad in UNUSABLE:
        pad = [0.0] * (4 - len(bad))
        sc, _ = step(Blab, 4, dict(BASE), rr, bad + pad, tol=0.75)  # converging with an unusable rho': converged, no breakdown
        assert same(sc, dict(moved, converged=1, stop=1)), bad
        sc, h = step(Blab, 4, dict(BASE), rr, bad + pad, tol=1e-6)  # not converging: breakdown, beta and rho untouched
        assert same(sc, dict(moved, breakdown=3, stop=1)) and h[4] == 4.0, bad
