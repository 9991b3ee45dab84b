"""The batched preconditioned solver's kernels (csrc/pcg_multi.hip) one at a time, for every k = 1..8, through the LAB build's
spmv_amd_pcg_multi_stage -- the launches spmv_amd_pcg_solve_device_multi makes, on caller data. Element-wise results are BIT-exact
against the oracle's fma forms for kinds "none", "jacobi" and "chebyshev"; both partial sets are BIT-equal to the restatement of
block_partials (tests/multi_rhs_restatement.py) computed from the column's own data -- so a column has the same bits whatever k is
and whatever slot it sits in; the reduction's totals are BIT-equal to reduce_multi; every scalar step is read field by field on
totals that are exactly representable. Every array lies between sentinel doubles that must survive each call (Guarded), and what a
stage only reads comes back unchanged. Column states -- frozen, converging in this iteration, skip_update -- are each tried in slot
0, slot 1 (the other half of slot 0's 16-byte pair) and the last slot."""
import numpy as np
import pytest

import multi_rhs_restatement as M
import reduction_restatement as RR
from bitwise import same_bits
from test_multi_rhs_stages_gpu import columns_of, interleave
from test_pcg_stages_gpu import Guarded

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
SIZES = [1, 2, 255, 256, 257, 1000, 4097]      # a lone tail row, whole workgroups, a tail of 1 (workgroup = 256 rows)
COUNTS = [1, 255, 256, 257, 4096, 4097, 8193]  # the slice is 4096 partials: one slice, an exact one, a short last, three
KINDS = ["none", "jacobi", "chebyshev", "chebyshev-last"]  # -last: term 0 is the whole polynomial, the r.z partials are written
COL = np.dtype([("rz", "f8"), ("pAp", "f8"), ("alpha", "f8"), ("beta", "f8"), ("b_norm", "f8"), ("residual", "f8"), ("active", "i4"),
                ("done", "i4"), ("iterations", "i4"), ("converged", "i4"), ("breakdown", "i4"), ("skip_update", "i4"), ("pad", "i4", 2)])
assert COL.itemsize == 80
C0, G, H = 0.6180339887, 1.4142135623, 0.5772156649
FILL = -7.25  # what an output array holds before the launch: a value no result has


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


def column_data(n, c):
    """The vectors and scalars of column id c at size n: a column's data never depends on k or on its slot."""
    rng = np.random.default_rng(100 * n + c)
    v = {name: rng.standard_normal(n) for name in ("R", "AP", "P", "X", "D", "Z")}
    v["alpha"], v["beta"] = float(rng.uniform(0.25, 2.0)) * (-1.0) ** c, float(rng.uniform(0.25, 2.0))
    return v


def dinv_of(n):
    return np.random.default_rng(n).uniform(0.5, 2.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)


STATES = {"live": dict(active=1), "frozen": dict(active=0, done=1, converged=1), "converging": dict(active=1, done=1, converged=1),
          "skip": dict(active=1, skip_update=1), "skip-stopped": dict(active=1, skip_update=1, done=1, breakdown=1)}


def scenarios(k, special):
    """Every slot live; then each special state at slot 0, slot 1 and the last slot."""
    out = [["live"] * k]
    for state in special:
        for slot in sorted({0, min(1, k - 1), k - 1}):
            row = ["live"] * k
            row[slot] = state
            out.append(row)
    return out


def records(data, states):
    c = np.zeros(len(states), dtype=COL)
    for s, state in enumerate(states):
        c[s]["alpha"], c[s]["beta"], c[s]["rz"], c[s]["b_norm"] = data[s]["alpha"], data[s]["beta"], 1.5, 2.5
        for name, v in STATES[state].items():
            c[s][name] = v
    return c


def z_of(O, kind, dinv, r):
    return r.copy() if kind == "none" else dinv * r if kind == "jacobi" else C0 * (dinv * r)


def run_stage(Blab, stage, kind, k, n, ids, states, last=0):
    """One launch on the columns `ids` in the states `states`; returns the arrays afterwards (k, n), the partials (2, k, count), the
    columns' data and dinv. Everything the stage does not write must come back unchanged -- checked by the caller against `data`."""
    base = "chebyshev" if kind.startswith("chebyshev") else kind
    data = [column_data(n, c) for c in ids]
    dinv = dinv_of(n)
    count = (n + 255) // 256
    host = {name: interleave([d[name] for d in data]) for name in ("R", "AP", "P", "X", "D", "Z")}
    dev = {name: Guarded(Blab, v) for name, v in host.items()}
    cols = records(data, states)
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    ddinv = Guarded(Blab, dinv)
    dpart = Guarded(Blab, np.full(2 * k * count, FILL))
    a = Blab.PcgMultiStageArgs(n=n, X=dev["X"].ptr, R=dev["R"].ptr, P=dev["P"].ptr, AP=dev["AP"].ptr, D=dev["D"].ptr, Z=dev["Z"].ptr,
                               dinv=ddinv.ptr, cols=dcols.ptr, partials=dpart.ptr, c0=C0, g=G, h=H, last=last)
    assert Blab.pcg_multi_stage(stage, base, k, a) == 0
    assert a.count == count
    out = {name: columns_of(v.read(), k) for name, v in dev.items()}
    out["partials"] = dpart.read().reshape(2, k, count)
    assert same_bits(dcols.read(), cols.view(np.float64)), "the column records are read only"
    assert same_bits(ddinv.read(), dinv), "dinv is read only"
    for v in list(dev.values()) + [dcols, ddinv, dpart]:
        v.free()
    return out, data, dinv


def unchanged(out, data, names, s, label):
    for name in names:
        assert same_bits(out[name][s], data[s][name]), (label, name, "changed")


def check_partials(out, s, n, rr, rz, label):
    """rr / rz: the column's products per row, or None where the launch must leave the set alone."""
    for v, prod in enumerate((rr, rz)):
        got = out["partials"][v][s]
        if prod is None:
            assert np.all(got == FILL), (label, v, "written")
        else:
            assert same_bits(got, M.block_partials_of(prod, M.flat())), (label, v)


def ids_for(k, rot):
    return [(s + rot) % 8 for s in range(k)]


# ---------------------------------------------------------------- init
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, O, n, kind):
    cheb, last = kind.startswith("chebyshev"), int(kind == "chebyshev-last")
    for k in KS:
        ids = ids_for(k, k)
        out, data, dinv = run_stage(Blab, "init", kind, k, n, ids, ["live"] * k, last)
        for s in range(k):
            label = (n, kind, k, s)
            r = O.axpy(-1.0, data[s]["AP"], data[s]["R"])
            z = z_of(O, kind[:9] if cheb else kind, dinv, r)
            assert same_bits(out["R"][s], r), label
            if cheb:
                assert same_bits(out["D"][s], z) and same_bits(out["Z"][s], z), label
                unchanged(out, data, ("AP", "P", "X"), s, label)
            else:
                assert same_bits(out["P"][s], z), label
                unchanged(out, data, ("AP", "X", "D", "Z"), s, label)
            check_partials(out, s, n, r * r, r * z if (not cheb or last) else None, label)


# ---------------------------------------------------------------- update_r
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_r_stage(Blab, O, n, kind):
    cheb, last = kind.startswith("chebyshev"), int(kind == "chebyshev-last")
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "skip"))):
            ids = ids_for(k, rot)
            out, data, dinv = run_stage(Blab, "update_r", kind, k, n, ids, states, last)
            for s, state in enumerate(states):
                label = (n, kind, k, tuple(states), s)
                d = data[s]
                r = O.axpy(-d["alpha"], d["AP"], d["R"]) if state == "live" else d["R"]
                z = z_of(O, kind[:9] if cheb else kind, dinv, r)
                assert same_bits(out["R"][s], r), label  # a frozen and a skip_update column keep every bit of r
                if cheb and state != "frozen":
                    assert same_bits(out["D"][s], z) and same_bits(out["Z"][s], z), label
                    unchanged(out, data, ("AP", "P", "X"), s, label)
                else:
                    unchanged(out, data, ("AP", "P", "X", "D", "Z"), s, label)
                check_partials(out, s, n, r * r, r * z if (not cheb or last) else None, label)


# ---------------------------------------------------------------- update_xp
@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("n", SIZES)
def test_update_xp_stage(Blab, O, n, kind):
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "converging", "skip-stopped"))):
            ids = ids_for(k, rot)
            out, data, dinv = run_stage(Blab, "update_xp", kind, k, n, ids, states)
            for s, state in enumerate(states):
                label = (n, kind, k, tuple(states), s)
                d = data[s]
                z = d["Z"] if kind == "chebyshev" else z_of(O, kind, dinv, d["R"])
                x = O.axpy(d["alpha"], d["P"], d["X"]) if state in ("live", "converging") else d["X"]
                p = O.axpy(d["beta"], d["P"], z) if state == "live" else d["P"]
                # frozen: every bit stays; converging: the x update, p stays; skip_update: x and p stay
                assert same_bits(out["X"][s], x) and same_bits(out["P"][s], p), label
                unchanged(out, data, ("R", "AP", "D", "Z"), s, label)
            assert np.all(out["partials"] == FILL)


# ---------------------------------------------------------------- cheb_step
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_cheb_step_stage(Blab, O, n, last):
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "converging")) + [["frozen"] * k]):
            ids = ids_for(k, rot)
            out, data, dinv = run_stage(Blab, "cheb_step", "chebyshev", k, n, ids, states, last)
            everyone_done = all(state != "live" for state in states)
            for s, state in enumerate(states):
                label = (n, last, k, tuple(states), s)
                d = data[s]
                if state == "live":
                    dd = O.axpy(G, dinv * O.axpy(-1.0, d["AP"], d["R"]), H * d["D"])
                    zz = d["Z"] + dd
                    assert same_bits(out["D"][s], dd) and same_bits(out["Z"][s], zz), label
                    unchanged(out, data, ("R", "AP", "P", "X"), s, label)
                    rz = d["R"] * zz
                else:  # done (frozen earlier, or stopped in this iteration): the step leaves every bit alone
                    unchanged(out, data, ("R", "AP", "P", "X", "D", "Z"), s, label)
                    rz = np.zeros(n)
                check_partials(out, s, n, None, rz if last and not everyone_done else None, label)


# ---------------------------------------------------------------- reduce
def run_reduce(Blab, k, partials, which, cols, tol=1e-6, hist_cap=8, hist_fill=FILL):
    """partials: (values, k, count). Returns the records and the (k, hist_cap) histories afterwards."""
    count = partials.shape[2]
    dpart = Guarded(Blab, partials.ravel())
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    dhist = Guarded(Blab, np.full(k * hist_cap, hist_fill))
    a = Blab.PcgMultiStageArgs(partials=dpart.ptr, cols=dcols.ptr, count=count, which=which, tol=tol, hist=dhist.ptr, hist_cap=hist_cap)
    assert Blab.pcg_multi_stage("reduce", None, k, a) == 0
    got = dcols.read().view(COL).copy()
    hist = dhist.read().reshape(k, hist_cap)
    assert same_bits(dpart.read(), partials.ravel())
    for v in (dpart, dcols, dhist):
        v.free()
    return got, hist


@pytest.mark.parametrize("count", COUNTS)
def test_reduce_totals_are_reduce_multi(Blab, count):
    """Both values of step 0 (||r0|| = sqrt of value 0's total, rz = value 1's) and the one of step 1 (pAp), every k."""
    rng = np.random.default_rng(count)
    pool = rng.standard_normal((2, 8, count))
    pool[0] = pool[0] ** 2
    want = [[RR.reduce_multi(pool[v][c]) for c in range(8)] for v in range(2)]
    for k in KS:
        ids = ids_for(k, k)
        got, hist = run_reduce(Blab, k, pool[:, ids, :].copy(), 0, np.zeros(k, dtype=COL))
        for s, c in enumerate(ids):
            assert same_bits(got[s]["b_norm"], np.sqrt(want[0][c])) and same_bits(got[s]["rz"], want[1][c]), (count, k, s)
            assert same_bits(hist[s][0], np.sqrt(want[0][c])) and np.all(hist[s][1:] == FILL)
        cols = np.zeros(k, dtype=COL)
        cols["rz"] = 3.0
        got, _ = run_reduce(Blab, k, pool[1:, ids, :].copy(), 1, cols)
        for s, c in enumerate(ids):
            assert got[s]["active"] == 1 and same_bits(got[s]["pAp"], want[1][c]) and same_bits(got[s]["alpha"], 3.0 / np.float64(want[1][c]))


def integer_partials(totals, count=300):
    """(len(totals), count) integer-valued partials with the given exact totals (a non-finite total: one such partial)."""
    out = np.zeros((len(totals), count))
    for j, t in enumerate(totals):
        if np.isfinite(t):
            out[j, :3] = (t - 7.0, 3.0, 4.0)
        else:
            out[j, 5] = t
    return out


def column(**fields):
    c = np.zeros(1, dtype=COL)[0]
    for name, v in fields.items():
        c[name] = v
    return c


def cols_of(columns):
    out = np.zeros(len(columns), dtype=COL)
    for j, c in enumerate(columns):
        out[j] = c
    return out


def fields_equal(got, want, label):
    for name in COL.names:
        if name == "pad":
            continue
        g, w = got[name], want[name]
        same = (np.isnan(g) and np.isnan(w)) or same_bits(np.float64(g), np.float64(w)) if COL[name].kind == "f" else g == w
        assert same, (label, name, g, w)


def test_scalar_steps_field_by_field(Blab):
    """Integer-valued partials: every total is exact. One column per case, all cases of a step in one launch of up to 8 columns."""
    tol = 0.25
    started = dict(rz=8.0, b_norm=4.0, residual=4.0, iterations=2)
    # step 0: everything is set afresh
    got, hist = run_reduce(Blab, 1, np.stack([integer_partials([16.0]), integer_partials([12.0])]), 0, cols_of([column(done=1, iterations=9, skip_update=1)]))
    fields_equal(got[0], column(b_norm=4.0, residual=4.0, rz=12.0), "step 0")
    assert hist[0][0] == 4.0 and np.all(hist[0][1:] == FILL)
    # step 1: a done column is not looked at; a usable pAp; zero, infinite and NaN ones
    before = [column(done=1, active=1, alpha=5.0, **started), column(**started), column(**started), column(**started), column(**started)]
    totals = [2.0, 2.0, 0.0, np.inf, np.nan]
    got, _ = run_reduce(Blab, 5, integer_partials(totals)[None], 1, cols_of(before))
    fields_equal(got[0], column(done=1, active=0, alpha=5.0, **started), "step 1 done")
    fields_equal(got[1], column(active=1, pAp=2.0, alpha=4.0, **started), "step 1 usable")
    for j in (2, 3, 4):
        fields_equal(got[j], column(active=1, pAp=totals[j], alpha=0.0, skip_update=1, **started), ("step 1 unusable", j))
    # steps 2 and 3: inactive; skip_update -> breakdown; the strict test (res / b_norm = 0.25 is NOT below tol = 0.25; 0.1875 is);
    # step 2 alone: an unusable r.z' -> breakdown, else beta and rz
    live = dict(active=1, alpha=4.0, pAp=2.0, **started)
    before = [column(active=0, done=1, **started), column(skip_update=1, **live), column(**live), column(**live), column(**live), column(**live),
              column(**live)]
    rr = [9.0, 9.0, 1.0, 0.5625, 9.0, 9.0, 9.0]
    rzn = [4.0, 4.0, 4.0, 4.0, 0.0, -np.inf, 4.0]
    for which in (2, 3):
        parts = np.stack([integer_partials(rr), integer_partials(rzn)]) if which == 2 else integer_partials(rr)[None]
        got, hist = run_reduce(Blab, 7, parts, which, cols_of(before), tol=tol, hist_cap=4)
        after = dict(live, iterations=3)
        fields_equal(got[0], before[0], (which, "inactive"))
        fields_equal(got[1], column(**dict(after, skip_update=1, residual=3.0, breakdown=1, done=1)), (which, "skip_update"))
        fields_equal(got[2], column(**dict(after, residual=1.0)) if which == 3 else column(**dict(after, residual=1.0, beta=0.5, rz=4.0)), (which, "at tol"))
        fields_equal(got[3], column(**dict(after, residual=0.75, converged=1, done=1)), (which, "below tol"))
        for j in (4, 5):
            want = dict(after, residual=3.0) if which == 3 else dict(after, residual=3.0, breakdown=1, done=1)
            fields_equal(got[j], column(**want), (which, "unusable r.z'", j))
        fields_equal(got[6], column(**dict(after, residual=3.0)) if which == 3 else column(**dict(after, residual=3.0, beta=0.5, rz=4.0)), (which, "goes on"))
        assert np.all(hist[0] == FILL) and hist[1][3] == 3.0 and hist[3][3] == 0.75 and np.all(hist[1:, :3] == FILL)
        # the history guard iterations < hist_cap: iteration 3 does not fit a history of 3
        got, hist = run_reduce(Blab, 7, parts, which, cols_of(before), tol=tol, hist_cap=3)
        assert np.all(hist == FILL) and got[6]["iterations"] == 3 and got[6]["residual"] == 3.0
    # step 4: r.z' and beta alone, for the columns still running
    going = dict(live, iterations=3, residual=3.0)
    before = [column(active=0, done=1, **started), column(**dict(going, converged=1, done=1)), column(**going), column(**going), column(**going)]
    totals = [4.0, 4.0, 4.0, 0.0, np.nan]
    got, _ = run_reduce(Blab, 5, integer_partials(totals)[None], 4, cols_of(before), tol=tol)
    fields_equal(got[0], before[0], "step 4 inactive")
    fields_equal(got[1], before[1], "step 4 stopped")
    fields_equal(got[2], column(**dict(going, beta=0.5, rz=4.0)), "step 4 goes on")
    for j in (3, 4):
        fields_equal(got[j], column(**dict(going, breakdown=1, done=1)), ("step 4 unusable", j))
