"""The GCR solver's kernels (csrc/gcr.hip) one at a time, through the LAB build's spmv_amd_gcr_stage -- the launches
spmv_amd_gcr_solve_device makes, on caller data -- against the restatement, BIT for bit: element-wise results against the oracle's
fma, the partials against reduction_restatement.stream_partials, the sums against reduce_pcg, the scalar step field by field in each
of its branches. Every vector lies inside a larger buffer with NaN in front and behind; the padding and the read-only inputs must
keep their bits, basis slots the kernel has no business with hold NaN that must reach no output, and a kernel launched behind a set
verdict must change no bit of anything."""
import ctypes as C

import numpy as np
import pytest

import reduction_restatement as R

pytestmark = pytest.mark.gpu

# an odd tail alone, one pair, pair + tail, 63 pairs + tail, one full wave, a wave + tail, 2 * 64 * 5 + 1: five full workgroups and
# the tail, and several workgroups with a tail
SIZES = [1, 2, 3, 127, 128, 129, 641, 4225]
KINDS = ["none", "jacobi"]
COUNTS = [1, 1024, 1025, 70_000]  # one workgroup, its largest, the first two-stage one, slice 274 in 256 slices with the last short
GUARD = 16
MAX = 32


def slots_around(chunk, lowest):
    """The first slots, the last one, and the slots on either side of each chunk boundary of a kernel that walks the basis `chunk`
    slots at a time (lab.h states the chunk sizes; csrc/gcr.hip asserts they are the kernels')."""
    s = {lowest, 1, 2, MAX - 1}
    for edge in range(chunk, MAX, chunk):
        s |= {edge - 1, edge, edge + 1}
    return sorted(j for j in s if lowest <= j < MAX)


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


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
    """The vectors of a stage call from `values` (name -> array; a name left out is a null pointer), the basis from Q and Z (lists of
    32 arrays) and a NaN partials buffer 32 values wide."""

    def __init__(self, Blab, n, kind, Q=None, Z=None, alias=None, **values):
        self.B, self.n, self.kind = Blab, n, kind
        self.count = R.stream_count(n)
        self.g = {k: Guarded(Blab, v) for k, v in values.items()}
        self.g["partials"] = Guarded(Blab, np.full(MAX * self.count, np.nan))
        self.args = Blab.GcrStageArgs(n=n, **{k: g.ptr for k, g in self.g.items()})
        for name, vectors in (("Q", Q), ("Z", Z)):
            if vectors is not None:
                for i, v in enumerate(vectors):
                    self.g[f"{name}{i}"] = Guarded(Blab, v)
                arr = (C.c_void_p * MAX)(*[self.g[f"{name}{i}"].ptr for i in range(MAX)])
                setattr(self, "_" + name, arr)  # keep the host array alive
                setattr(self.args, name, arr)
        if alias is not None:  # alias = (field, name): the field points at a vector that is already there
            setattr(self.args, alias[0], self.g[alias[1]].ptr)

    def run(self, stage, scalars=None):
        assert self.B.gcr_stage(stage, self.kind, self.args, scalars) == 0
        assert self.args.count == self.count
        return {k: g.read() for k, g in self.g.items()}

    def only_changed(self, *names):
        return all(g.untouched() for k, g in self.g.items() if k not in names)

    def free(self):
        for g in self.g.values():
            g.free()


def fma(O, a, u, c):
    return O.fma(np.full(len(u), a), u, c)


def scalars(Blab, beta=(), gamma=(), **kw):
    sc = Blab.GcrScalars()
    for i in range(MAX):
        sc.gamma[i] = sc.beta[i] = np.nan
    for i, v in enumerate(beta):
        sc.beta[i] = v
    for i, v in enumerate(gamma):
        sc.gamma[i] = v
    base = dict(alpha=np.nan, rho=np.nan, b_norm=np.nan, residual=np.nan)
    base.update(kw)
    for k, v in base.items():
        setattr(sc, k, v)
    return sc


def basis(rng, n, filled):
    """32 vectors: the first `filled` random, the rest NaN."""
    return [rng.standard_normal(n) if i < filled else np.full(n, np.nan) for i in range(MAX)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, n, kind):
    """r = fma(1.0, b, -1.0 * v) (the difference rounded once), the partials of r.r; "jacobi": zs = dinv r."""
    rng = np.random.default_rng(1000 * n + 1)
    d = dict(b=rng.standard_normal(n), v=rng.standard_normal(n), r=np.full(n, np.nan))
    if kind == "jacobi":
        d.update(dinv=rng.choice([-1.0, 1.0]) / rng.uniform(0.5, 4.0, n), zs=np.full(n, np.nan))
    s = Stage(Blab, n, kind, **d)
    got = s.run("init")
    want = d["b"] - d["v"]
    assert same_bits(got["r"], want)
    if kind == "jacobi":
        assert same_bits(got["zs"], d["dinv"] * want)
    assert same_bits(got["partials"][:s.count], R.stream_partials(want, want)) and np.all(np.isnan(got["partials"][s.count:]))
    assert s.only_changed("r", "zs", "partials")
    s.free()


@pytest.mark.parametrize("n", SIZES)
def test_multidot_stage(Blab, n):
    """Value i < j of the partials is stream_partials(Q_i, Q_j) -- the bits bicg_dot_kernel<false> gives for that pair --, whatever
    chunk slot i falls into; slots > j hold NaN and nothing past value j - 1 is written; behind a verdict nothing at all."""
    for j in slots_around(Blab.GCR_DOT_CHUNK, 1):
        rng = np.random.default_rng(1000 * n + 50 + j)
        Q = basis(rng, n, j + 1)
        s = Stage(Blab, n, None, Q=Q)
        s.args.slot = j
        s.run("multidot", scalars(Blab, stop=1))
        assert s.only_changed(), j
        got = s.run("multidot", scalars(Blab))["partials"]
        for i in range(j):
            assert same_bits(got[i * s.count:(i + 1) * s.count], R.stream_partials(Q[i], Q[j])), (j, i)
        assert np.all(np.isnan(got[j * s.count:])) and s.only_changed("partials"), j
        s.free()


@pytest.mark.parametrize("z_is_r", [True, False], ids=["z-is-r", "z-apart"])
@pytest.mark.parametrize("n", SIZES)
def test_orthogonalise_stage(Blab, O, n, z_is_r):
    """q = Q_j and z = z_in, then for i ascending q = fma(-beta_i, Q_i, q), z = fma(-beta_i, Z_i, z); Q_j in place (untouched at
    j = 0), Z_j out of place, the partials of q.q and r.q. z_in is r itself (kind "none") or a vector apart (every other kind). Slots
    > j hold NaN; behind a verdict nothing at all."""
    for j in slots_around(Blab.GCR_ORTH_CHUNK, 0):
        rng = np.random.default_rng(1000 * n + 100 + j)
        Q, Z = basis(rng, n, j + 1), basis(rng, n, j)
        beta = rng.uniform(-2.0, 2.0, j)
        d = dict(r=rng.standard_normal(n))
        if not z_is_r:
            d["z_in"] = rng.standard_normal(n)
        s = Stage(Blab, n, None, Q=Q, Z=Z, alias=("z_in", "r") if z_is_r else None, **d)
        s.args.slot = j
        s.run("orthogonalise", scalars(Blab, beta=beta, stop=1))
        assert s.only_changed(), j
        got = s.run("orthogonalise", scalars(Blab, beta=beta))
        q, z = Q[j], d["r"] if z_is_r else d["z_in"]
        for i in range(j):
            q, z = fma(O, -beta[i], Q[i], q), fma(O, -beta[i], Z[i], z)
        assert same_bits(got[f"Q{j}"], q) and same_bits(got[f"Z{j}"], z), j
        want = np.concatenate([R.stream_partials(q, q), R.stream_partials(d["r"], q)])
        assert same_bits(got["partials"][:2 * s.count], want) and np.all(np.isnan(got["partials"][2 * s.count:])), j
        assert s.only_changed(*((f"Q{j}",) if j > 0 else ()), f"Z{j}", "partials"), j
        s.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xr_stage(Blab, O, n, kind):
    """x = fma(alpha, Z_j, x), r = fma(-alpha, Q_j, r), the partials of r.r; "jacobi": zs = dinv r. Only slot j of the basis is
    looked at (every other slot holds NaN); behind a verdict nothing at all."""
    for j in (0, 1, 2, MAX - 1):
        rng = np.random.default_rng(1000 * n + 200 + j)
        Q = [rng.standard_normal(n) if i == j else np.full(n, np.nan) for i in range(MAX)]
        Z = [rng.standard_normal(n) if i == j else np.full(n, np.nan) for i in range(MAX)]
        d = dict(x=rng.standard_normal(n), r=rng.standard_normal(n))
        if kind == "jacobi":
            d.update(dinv=rng.choice([-1.0, 1.0]) / rng.uniform(0.5, 4.0, n), zs=np.full(n, np.nan))
        alpha = float(rng.uniform(-2.0, 2.0))
        s = Stage(Blab, n, kind, Q=Q, Z=Z, **d)
        s.args.slot = j
        s.run("update_xr", scalars(Blab, alpha=alpha, stop=1))
        assert s.only_changed(), j
        got = s.run("update_xr", scalars(Blab, alpha=alpha))
        want_r = fma(O, -alpha, Q[j], d["r"])
        assert same_bits(got["x"], fma(O, alpha, Z[j], d["x"])) and same_bits(got["r"], want_r), j
        if kind == "jacobi":
            assert same_bits(got["zs"], d["dinv"] * want_r), j
        assert same_bits(got["partials"][:s.count], R.stream_partials(want_r, want_r)) and np.all(np.isnan(got["partials"][s.count:])), j
        assert s.only_changed("x", "r", "zs", "partials"), j
        s.free()


# ---------------------------------------------------------------- the reducing launch
def reduce_stage(Blab, partials_ptr, count, which, incoming, slot=0, tol=0.0, hist_ptr=None, hist_cap=0):
    a = Blab.GcrStageArgs(partials=partials_ptr, count=count, which=which, slot=slot, tol=tol, hist=hist_ptr, hist_cap=hist_cap)
    assert Blab.gcr_stage("reduce", None, a, incoming) == 0
    return incoming


def fields(sc):
    out = {}
    for name, _ in sc._fields_:
        v = getattr(sc, name)
        out[name] = np.array(list(v)) if name in ("gamma", "beta") else v
    return out


def same(got, want):
    """two scalar records field by field, NaN equal to NaN, -0.0 not equal to 0.0"""
    return all(np.array_equal(bits(np.asarray(got[k], dtype=np.float64)), bits(np.asarray(want[k], dtype=np.float64))) for k in want)


@pytest.mark.parametrize("count", COUNTS)
def test_reduction_alone(Blab, count):
    """1, 2 and 31 values of `count` partials each against reduce_pcg, twice the same: one value through steps 0 and 3, slot values
    through step 1 (beta_i = total_i / gamma_i, the slots from `slot` on untouched), two through step 2; a sum behind a verdict
    changes no field."""
    rng = np.random.default_rng(count)
    values = rng.standard_normal((MAX - 1, count))
    values[0] = values[0] ** 2
    buf = Guarded(Blab, values.ravel())
    totals = [np.float64(t) for t in R.reduce_pcg(values.ravel(), count, MAX - 1)]
    gamma = rng.uniform(0.5, 2.0, MAX) * rng.choice([-1.0, 1.0], MAX)
    for _ in range(2):
        sc = reduce_stage(Blab, buf.ptr, count, 0, scalars(Blab))
        assert bits(sc.b_norm) == bits(np.sqrt(totals[0])) and bits(sc.residual) == bits(np.sqrt(totals[0])) and sc.iterations == 0
        sc = reduce_stage(Blab, buf.ptr, count, 3, scalars(Blab, b_norm=1.0))
        assert bits(sc.residual) == bits(np.sqrt(totals[0])) and sc.iterations == 1 and sc.stop == 0
        for nv in (1, 2, MAX - 1):
            sc = reduce_stage(Blab, buf.ptr, count, 1, scalars(Blab, gamma=gamma), slot=nv)
            got = np.array(list(sc.beta))
            assert same_bits(got[:nv], np.array([totals[i] / np.float64(gamma[i]) for i in range(nv)])), nv
            assert np.all(np.isnan(got[nv:])) and same_bits(np.array(list(sc.gamma)), gamma), nv
        sc = reduce_stage(Blab, buf.ptr, count, 2, scalars(Blab, gamma=gamma), slot=5)
        assert bits(sc.gamma[5]) == bits(totals[0]) and bits(sc.rho) == bits(totals[1]) and bits(sc.alpha) == bits(totals[1] / totals[0])
        assert same_bits(np.delete(np.array(list(sc.gamma)), 5), np.delete(gamma, 5)) and sc.stop == 0
    for which in (1, 2, 3):
        kw = dict(gamma=gamma, beta=gamma[::-1], alpha=0.5, rho=3.0, b_norm=1.0, residual=2.0, iterations=3, stop=1, converged=1)
        after = reduce_stage(Blab, buf.ptr, count, which, scalars(Blab, **kw), slot=2)
        assert same(fields(after), fields(scalars(Blab, **kw))), which
    assert buf.untouched()
    buf.free()


def step(Blab, which, incoming, v0, v1=None, slot=0, tol=0.0, hist_cap=8):
    """One reduce + step over exactly representable partials; returns the outgoing record and the 8-entry history buffer."""
    v0 = np.asarray(v0, dtype=np.float64)
    part = Guarded(Blab, v0 if v1 is None else np.concatenate([v0, np.asarray(v1, dtype=np.float64)]))
    hist = Guarded(Blab, np.full(8, -7.0))
    sc = reduce_stage(Blab, part.ptr, len(v0), which, scalars(Blab, **incoming), slot, tol, hist.ptr, hist_cap)
    h = hist.read()
    part.free(), hist.free()
    return fields(sc), h


GAMMA = np.array([2.0 ** (i % 5) for i in range(MAX)])
BETA = np.array([0.25 * (i + 1) for i in range(MAX)])
BASE = dict(gamma=GAMMA, beta=BETA, alpha=0.5, rho=3.0, b_norm=8.0, residual=2.0, iterations=3, converged=0, breakdown=0, stop=0)
UNUSABLE = ([0.0], [-0.0], [1.0, -1.0], [np.inf], [-np.inf], [np.nan], [np.inf, -np.inf], [1.0, np.nan, 2.0])
QUIET = np.full(8, -7.0)


def recorded(slot, value):
    h = QUIET.copy()
    h[slot] = value
    return h


def with_slot(a, j, v):
    a = a.copy()
    a[j] = v
    return a


def test_step_0_initial_scalars(Blab):
    garbage = dict(gamma=np.full(MAX, 7.0), beta=np.full(MAX, 7.0), alpha=7.0, rho=7.0, b_norm=7.0, residual=7.0, iterations=7, converged=7,
                   breakdown=7, stop=7)
    for cap in (0, 1, 8):
        sc, h = step(Blab, 0, garbage, [4.0, 4.0, 4.0, 4.0], hist_cap=cap)
        assert same(sc, dict(gamma=np.zeros(MAX), beta=np.zeros(MAX), alpha=0.0, rho=0.0, b_norm=4.0, residual=4.0, iterations=0,
                             converged=0, breakdown=0, stop=0))
        assert np.array_equal(h, recorded(0, 4.0) if cap else QUIET)


def test_step_1_the_betas(Blab):
    """beta_i = total_i / gamma_i for i < slot and nothing else: no verdict, no history; a zero gamma gives the IEEE quotient."""
    sc, h = step(Blab, 1, dict(BASE), [1.0, 2.0], [-7.0, 0.5], slot=2)  # two values of two partials: 3 and -6.5
    assert same(sc, dict(BASE, beta=with_slot(with_slot(BETA, 0, 3.0 / GAMMA[0]), 1, -6.5 / GAMMA[1]))) and np.array_equal(h, QUIET)
    sc, _ = step(Blab, 1, dict(BASE, gamma=with_slot(GAMMA, 0, 0.0)), [1.0], slot=1)
    assert np.isinf(sc["beta"][0]) and sc["stop"] == 0 and sc["iterations"] == 3


def test_step_2_alpha_and_the_breakdowns(Blab):
    for j, qq, rq in ((0, [1.0, 3.0], [1.0, 2.0]), (5, [7.0], [-3.0]), (31, [1.0, 2.0], [-8.0, 2.0])):
        g, r = np.float64(sum(qq)), np.float64(sum(rq))
        sc, h = step(Blab, 2, dict(BASE), qq, rq, slot=j)  # a negative rho is an ordinary value
        assert same(sc, dict(BASE, gamma=with_slot(GAMMA, j, g), rho=r, alpha=r / g)) and np.array_equal(h, QUIET), j
    for bad in UNUSABLE:  # the iteration is counted, the unchanged residual recorded, nothing will be updated
        for which, qq, rq in ((1, bad, [2.0] * len(bad)), (2, [2.0] * len(bad), bad), (1, bad, bad)):
            sc, h = step(Blab, 2, dict(BASE), qq, rq, slot=3)
            want = dict(BASE, alpha=0.0, breakdown=which, stop=1, iterations=4)
            assert same({k: v for k, v in sc.items() if k != "rho"}, {k: v for k, v in want.items() if k != "rho"}), (qq, rq)
            assert np.array_equal(h, recorded(4, 2.0)), (qq, rq)
    sc, h = step(Blab, 2, dict(BASE), [0.0], [1.0], hist_cap=4)  # hist_cap reached: counted, not written
    assert sc["iterations"] == 4 and sc["breakdown"] == 1 and sc["stop"] == 1 and np.array_equal(h, QUIET)


def test_step_3_history_and_verdict(Blab):
    rr = [4.0, 4.0, 4.0, 4.0]  # ||r|| = 4, ||r0|| = 8: 0.5
    moved = dict(BASE, iterations=4, residual=4.0)
    for cap, written in ((8, True), (5, True), (4, False), (3, False), (0, False)):  # a capacity of exactly `iterations` writes nothing
        sc, h = step(Blab, 3, dict(BASE), rr, tol=1e-6, hist_cap=cap)
        assert same(sc, moved) and np.array_equal(h, recorded(4, 4.0) if written else QUIET), cap
    sc, _ = step(Blab, 3, dict(BASE), rr, tol=0.5)  # STRICT: equal to tol goes on
    assert same(sc, moved)
    for cap, written in ((8, True), (4, False)):
        sc, h = step(Blab, 3, dict(BASE), rr, tol=float(np.nextafter(0.5, 1.0)), hist_cap=cap)
        assert same(sc, dict(moved, converged=1, stop=1)) and np.array_equal(h, recorded(4, 4.0) if written else QUIET), cap
    sc, _ = step(Blab, 3, dict(BASE), [np.nan], tol=1.0)  # NaN is not below anything
    assert sc["stop"] == 0 and sc["converged"] == 0 and np.isnan(sc["residual"]) and sc["iterations"] == 4
    sc, _ = step(Blab, 3, dict(BASE), [0.0], tol=0.0)  # nor is 0 below 0
    assert same(sc, dict(BASE, iterations=4, residual=0.0))
