"""The batched BiCGSTAB solver's kernels (csrc/bicgstab_multi.hip) one at a time, for every k = 1..8 and both kinds, through the LAB
build's spmv_amd_bicgstab_multi_stage -- the launches spmv_amd_bicgstab_solve_device_multi makes, on caller data. Element-wise results
are BIT-exact against the oracle's fma forms; every partial set is BIT-equal to the restatement of block_partials
(tests/multi_rhs_restatement.py) computed from the column's own data -- so a column has the same bits whatever k is and whatever slot
it sits in; the reduction's totals are BIT-equal to reduce_multi; every scalar step is read field by field on totals that are exactly
representable. Column records mix running columns, columns frozen earlier, and columns that stopped in this iteration with x_step 0
and 1, each tried in slot 0, slot 1 (the other half of slot 0's 16-byte pair) and the last slot. Whatever a stage does not work on
for a column is NaN-POISONED on entry: it must come back bit-identical, that column's partials must be 0.0 and no other column's
partial may change. Every array lies between sentinel doubles that must survive each call (Guarded)."""
import numpy as np
import pytest

import multi_rhs_restatement as M
import reduction_restatement as RR
from bitwise import same_bits
from test_multi_rhs_stages_gpu import columns_of, interleave
from test_pcg_stages_gpu import Guarded

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
SIZES = [1, 2, 255, 256, 257, 513]  # a lone row, one workgroup short by a row, exact, a tail of 1, three workgroups (workgroup = 256 rows)
COUNTS = [1, 4095, 4096, 4097]      # the slice is 4096 partials: one short slice, an exact one, a second of one partial
KINDS = ["none", "jacobi"]
VECTORS = ("X", "R", "RH", "P", "PH", "SH", "V", "T")
COL = np.dtype([("rho", "f8"), ("sigma", "f8"), ("alpha", "f8"), ("omega", "f8"), ("beta", "f8"), ("b_norm", "f8"), ("residual", "f8"),
                ("s_norm", "f8"), ("active", "i4"), ("done", "i4"), ("iterations", "i4"), ("converged", "i4"), ("breakdown", "i4"),
                ("x_step", "i4"), ("pad", "i4", 2)])
assert COL.itemsize == 96
FILL = -7.25  # what an output array holds before the launch: a value no result has

# live: running. frozen: stopped in an earlier iteration (x_step is stale: nothing may look at it). half: stopped in THIS iteration by
# the half step or the omega breakdown (x_step 1). sigma: stopped in this iteration by the sigma breakdown (x_step 0).
STATES = {"live": dict(active=1, x_step=2), "frozen": dict(active=0, done=1, converged=1, x_step=2),
          "half": dict(active=1, done=1, converged=1, x_step=1), "sigma": dict(active=1, done=1, breakdown=1, x_step=0)}


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


def column_data(n, c):
    """The vectors and scalars of column id c at size n: a column's data never depends on k or on its slot."""
    rng = np.random.default_rng(100 * n + c)
    v = {name: rng.standard_normal(n) for name in VECTORS}
    v["alpha"], v["omega"], v["beta"] = (float(rng.uniform(0.25, 2.0)) * (-1.0) ** c, float(rng.uniform(0.25, 2.0)),
                                         float(rng.uniform(0.25, 2.0)) * (-1.0) ** (c // 2))
    return v


def dinv_of(n):
    return np.random.default_rng(n).uniform(0.5, 2.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)


def scenarios(k, special):
    """Every slot live; then each special state at slot 0, slot 1 and the last slot; then nobody live."""
    out = [["live"] * k]
    for state in special:
        for slot in sorted({0, min(1, k - 1), k - 1}):
            row = ["live"] * k
            row[slot] = state
            out.append(row)
    out.append([special[0]] * k)
    return out


def records(data, states):
    c = np.zeros(len(states), dtype=COL)
    for s, state in enumerate(states):
        c[s]["alpha"], c[s]["omega"], c[s]["beta"], c[s]["rho"], c[s]["b_norm"] = data[s]["alpha"], data[s]["omega"], data[s]["beta"], 1.5, 2.5
        for name, v in STATES[state].items():
            c[s][name] = v
    return c


def ids_for(k, rot):
    return [(s + rot) % 8 for s in range(k)]


def run_stage(Blab, stage, kind, k, n, ids, states, poisoned):
    """One launch on the columns `ids` in the states `states`. poisoned(state) -> the names of the vectors that column's stage must
    not look at: they hold NaN on entry. Returns the arrays afterwards (k, n), the partials (2, k, count), the columns' data as they
    went in, and dinv. Kind "none" hands no PH and SH over: P and R serve."""
    jac = kind == "jacobi"
    data = [column_data(n, c) for c in ids]
    for d, state in zip(data, states):
        for name in poisoned(state):
            d[name] = np.full(n, np.nan)
    dinv = dinv_of(n)
    count = (n + 255) // 256
    names = [name for name in VECTORS if jac or name not in ("PH", "SH")]
    dev = {name: Guarded(Blab, interleave([d[name] for d in data])) for name in names}
    cols = records(data, states)
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    ddinv = Guarded(Blab, dinv)
    dpart = Guarded(Blab, np.full(2 * k * count, FILL))
    ptr = {name: v.ptr for name, v in dev.items()}
    a = Blab.BicgstabMultiStageArgs(n=n, dinv=ddinv.ptr if jac else None, cols=dcols.ptr, partials=dpart.ptr, **ptr)
    assert Blab.bicgstab_multi_stage(stage, kind, k, a) == 0
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
        if name in out:
            assert same_bits(out[name][s], data[s][name]), (label, name, "changed")


def check_partials(out, s, values, label):
    """values: per value the column's products per row, 0.0 for a column the launch passes over, or None where the launch must leave
    the set alone."""
    for v, prod in enumerate(values):
        got = out["partials"][v][s]
        if prod is None:
            assert np.all(got == FILL), (label, v, "written")
        else:
            n = len(out["R"][s])
            want = M.block_partials_of(np.broadcast_to(np.asarray(prod, dtype=np.float64), (n,)).copy(), M.flat())
            assert same_bits(got, want), (label, v)


# ---------------------------------------------------------------- init
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, O, n, kind):
    jac = kind == "jacobi"
    for k in KS:
        out, data, dinv = run_stage(Blab, "init", kind, k, n, ids_for(k, k), ["live"] * k, lambda state: ("RH", "P", "PH"))
        for s in range(k):
            label = (n, kind, k, s)
            r = O.axpy(-1.0, data[s]["V"], data[s]["R"])  # fma(1.0, b, -1.0 * Ax0): one rounding of b - Ax0
            assert same_bits(out["R"][s], r) and same_bits(out["RH"][s], r) and same_bits(out["P"][s], r), label
            if jac:
                assert same_bits(out["PH"][s], dinv * r), label
            unchanged(out, data, ("X", "V", "T", "SH"), s, label)
            check_partials(out, s, (r * r, None), label)


# ---------------------------------------------------------------- dot_rv
@pytest.mark.parametrize("n", SIZES)
def test_dot_rv_stage(Blab, n):
    """Before step 1: a column takes part when it is not done, whatever `active` still says."""
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "half"))):
            everyone_done = all(state != "live" for state in states)
            out, data, _ = run_stage(Blab, "dot_rv", "none", k, n, ids_for(k, rot), states,
                                     lambda state: () if state == "live" else VECTORS)
            for s, state in enumerate(states):
                label = (n, k, tuple(states), s)
                unchanged(out, data, VECTORS, s, label)
                prod = None if everyone_done else data[s]["RH"] * data[s]["V"] if state == "live" else 0.0
                check_partials(out, s, (prod, None), label)


# ---------------------------------------------------------------- update_s
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_s_stage(Blab, O, n, kind):
    jac = kind == "jacobi"
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "half", "sigma"))):
            nobody = all(state != "live" for state in states)
            out, data, dinv = run_stage(Blab, "update_s", kind, k, n, ids_for(k, rot), states,
                                        lambda state: ("X", "RH", "P", "PH", "SH", "T") if state == "live" else VECTORS)
            for s, state in enumerate(states):
                label = (n, kind, k, tuple(states), s)
                d = data[s]
                if state == "live":
                    sv = O.axpy(-d["alpha"], d["V"], d["R"])
                    assert same_bits(out["R"][s], sv), label
                    if jac:
                        assert same_bits(out["SH"][s], dinv * sv), label
                    unchanged(out, data, ("X", "RH", "P", "PH", "V", "T"), s, label)
                    check_partials(out, s, (sv * sv, None), label)
                else:  # stopped, earlier or in this iteration: every bit stays, S^ included
                    unchanged(out, data, VECTORS, s, label)
                    check_partials(out, s, (None if nobody else 0.0, None), label)


# ---------------------------------------------------------------- dot_t
@pytest.mark.parametrize("n", SIZES)
def test_dot_t_stage(Blab, n):
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "half", "sigma"))):
            nobody = all(state != "live" for state in states)
            out, data, _ = run_stage(Blab, "dot_t", "none", k, n, ids_for(k, rot), states,
                                     lambda state: ("X", "RH", "P", "V") if state == "live" else VECTORS)
            for s, state in enumerate(states):
                label = (n, k, tuple(states), s)
                unchanged(out, data, VECTORS, s, label)
                if nobody:
                    check_partials(out, s, (None, None), label)
                elif state == "live":
                    check_partials(out, s, (data[s]["T"] * data[s]["R"], data[s]["T"] * data[s]["T"]), label)
                else:
                    check_partials(out, s, (0.0, 0.0), label)


# ---------------------------------------------------------------- update_xr
def xr_poison(kind):
    jac = kind == "jacobi"
    whole = ("V",) + (("P",) if jac else ())                # a whole step reads x, p^, s, s^, t and r^0
    half = ("V", "R", "RH", "T", "SH") + (("P",) if jac else ())  # a half step reads x and p^ alone

    def poisoned(state):
        return whole if state == "live" else half if state == "half" else VECTORS
    return poisoned


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xr_stage(Blab, O, n, kind):
    jac = kind == "jacobi"
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "half", "sigma")) + [["half"] * k]):
            nobody_active = all(state == "frozen" for state in states)
            out, data, dinv = run_stage(Blab, "update_xr", kind, k, n, ids_for(k, rot), states, xr_poison(kind))
            for s, state in enumerate(states):
                label = (n, kind, k, tuple(states), s)
                d = data[s]
                ph = d["PH"] if jac else d["P"]
                if state == "live":
                    sh = d["SH"] if jac else d["R"]
                    x = O.axpy(d["omega"], sh, O.axpy(d["alpha"], ph, d["X"]))
                    r = O.axpy(-d["omega"], d["T"], d["R"])
                    assert same_bits(out["X"][s], x) and same_bits(out["R"][s], r), label
                    unchanged(out, data, ("RH", "P", "PH", "SH", "V", "T"), s, label)
                    check_partials(out, s, (r * r, d["RH"] * r), label)
                else:
                    x = O.axpy(d["alpha"], ph, d["X"]) if state == "half" else d["X"]
                    assert same_bits(out["X"][s], x), label
                    unchanged(out, data, ("R", "RH", "P", "PH", "SH", "V", "T"), s, label)
                    check_partials(out, s, (None, None) if nobody_active else (0.0, 0.0), label)


# ---------------------------------------------------------------- direction
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_direction_stage(Blab, O, n, kind):
    jac = kind == "jacobi"
    for k in KS:
        for rot, states in enumerate(scenarios(k, ("frozen", "half", "sigma"))):
            out, data, dinv = run_stage(Blab, "direction", kind, k, n, ids_for(k, rot), states,
                                        lambda state: ("X", "RH", "PH", "SH", "T") if state == "live" else VECTORS)
            for s, state in enumerate(states):
                label = (n, kind, k, tuple(states), s)
                d = data[s]
                if state == "live":
                    p = O.axpy(d["beta"], O.axpy(-d["omega"], d["V"], d["P"]), d["R"])
                    assert same_bits(out["P"][s], p), label
                    if jac:
                        assert same_bits(out["PH"][s], dinv * p), label
                    unchanged(out, data, ("X", "R", "RH", "SH", "V", "T"), s, label)
                else:  # stopped, earlier or in this iteration: P and P^ keep every bit
                    unchanged(out, data, VECTORS, s, label)
            assert np.all(out["partials"] == FILL)


# ---------------------------------------------------------------- reduce
def run_reduce(Blab, k, partials, which, cols, tol=1e-6, hist_cap=8):
    """partials: (values, k, count). Returns the records and the (k, hist_cap) histories afterwards."""
    count = partials.shape[2]
    dpart = Guarded(Blab, partials.ravel())
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    dhist = Guarded(Blab, np.full(k * hist_cap, FILL))
    a = Blab.BicgstabMultiStageArgs(partials=dpart.ptr, cols=dcols.ptr, count=count, which=which, tol=tol, hist=dhist.ptr, hist_cap=hist_cap)
    assert Blab.bicgstab_multi_stage("reduce", None, k, a) == 0
    got = dcols.read().view(COL).copy()
    hist = dhist.read().reshape(k, hist_cap)
    assert same_bits(dpart.read(), partials.ravel())
    for v in (dpart, dcols, dhist):
        v.free()
    return got, hist


@pytest.mark.parametrize("count", COUNTS)
def test_reduce_totals_are_reduce_multi(Blab, count):
    """Every `which` on random partials, every k, the columns rotated through the slots: step 0 (||r0|| and rho of value 0), step 1
    (sigma, alpha), step 2 (||s||), step 3 (omega = value 0 / value 1), step 4 (||r||, rho' of value 1, beta)."""
    rng = np.random.default_rng(count)
    pool = rng.standard_normal((2, 8, count))
    square = pool[0] ** 2
    want = [[RR.reduce_multi(pool[v][c]) for c in range(8)] for v in range(2)]
    want_sq = [RR.reduce_multi(square[c]) for c in range(8)]
    live = np.zeros(1, dtype=COL)[0]
    live["rho"], live["alpha"], live["omega"], live["b_norm"], live["active"], live["x_step"] = 3.0, 0.75, 1.25, 1e-300, 1, 2
    for k in KS:
        ids = ids_for(k, k)
        cols = np.zeros(k, dtype=COL)
        cols[:] = live
        label = (count, k)
        got, hist = run_reduce(Blab, k, square[None, ids, :].copy(), 0, cols)
        for s, c in enumerate(ids):
            assert same_bits(got[s]["rho"], want_sq[c]) and same_bits(got[s]["b_norm"], np.sqrt(want_sq[c])), label
            assert same_bits(hist[s][0], np.sqrt(want_sq[c])) and np.all(hist[s][1:] == FILL), label
        got, _ = run_reduce(Blab, k, pool[1:, ids, :].copy(), 1, cols)
        for s, c in enumerate(ids):
            assert same_bits(got[s]["sigma"], want[1][c]) and same_bits(got[s]["alpha"], 3.0 / np.float64(want[1][c])), label
        got, _ = run_reduce(Blab, k, square[None, ids, :].copy(), 2, cols, tol=0.0)
        for s, c in enumerate(ids):
            assert same_bits(got[s]["s_norm"], np.sqrt(want_sq[c])) and got[s]["done"] == 0, label
        got, _ = run_reduce(Blab, k, pool[:, ids, :].copy(), 3, cols)
        for s, c in enumerate(ids):
            assert same_bits(got[s]["omega"], np.float64(want[0][c]) / np.float64(want[1][c])) and got[s]["done"] == 0, label
        got, hist = run_reduce(Blab, k, np.stack([square[ids], pool[1][ids]]), 4, cols, tol=0.0)
        for s, c in enumerate(ids):
            beta = (np.float64(want[1][c]) / np.float64(3.0)) * (np.float64(0.75) / np.float64(1.25))
            assert same_bits(got[s]["residual"], np.sqrt(want_sq[c])) and same_bits(hist[s][1], np.sqrt(want_sq[c])), label
            assert same_bits(got[s]["rho"], want[1][c]) and same_bits(got[s]["beta"], beta) and got[s]["done"] == 0, label


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
    """Integer-valued partials: every total is exact. One column per case, all cases of a step in one launch of up to 8 columns.
    Every branch of bicgstab.hip's bicg_step, and for each step behind step 1 a frozen column and one that stopped in this iteration:
    neither is looked at."""
    tol = 0.25
    started = dict(rho=8.0, b_norm=4.0, residual=4.0, iterations=2)
    frozen = column(active=0, done=1, converged=1, alpha=5.0, x_step=2, **started)
    stopped = column(active=1, done=1, breakdown=1, x_step=0, **dict(started, iterations=3))
    # step 0: everything is set afresh
    got, hist = run_reduce(Blab, 1, integer_partials([16.0])[None], 0, cols_of([column(done=1, active=1, iterations=9, x_step=1, breakdown=2)]))
    fields_equal(got[0], column(rho=16.0, b_norm=4.0, residual=4.0), "step 0")
    assert hist[0][0] == 4.0 and np.all(hist[0][1:] == FILL)
    # step 1: a done column only loses `active`; a usable sigma; zero, infinite and NaN ones break down, counted and recorded
    before = [column(active=1, done=1, converged=1, alpha=5.0, x_step=2, **started)] + [column(**started)] * 4
    totals = [2.0, 2.0, 0.0, np.inf, np.nan]
    got, hist = run_reduce(Blab, 5, integer_partials(totals)[None], 1, cols_of(before), tol=tol, hist_cap=4)
    fields_equal(got[0], frozen, "step 1 done")
    fields_equal(got[1], column(active=1, sigma=2.0, alpha=4.0, x_step=2, **started), "step 1 usable")
    for j in (2, 3, 4):
        want = column(active=1, sigma=totals[j], alpha=0.0, x_step=0, breakdown=1, done=1, **dict(started, iterations=3))
        fields_equal(got[j], want, ("step 1 unusable", j))
        assert hist[j][3] == 4.0 and np.all(hist[j][:3] == FILL)
    assert np.all(hist[:2] == FILL)
    # step 2: the strict test (||s|| / ||r0|| = 0.25 is NOT below tol = 0.25; 0.1875 is); a NaN norm is not below anything
    live = dict(active=1, sigma=2.0, alpha=4.0, x_step=2, **started)
    before = [frozen, stopped, column(**live), column(**live), column(**live)]
    totals = [0.5625, 0.5625, 1.0, 0.5625, np.nan]
    got, hist = run_reduce(Blab, 5, integer_partials(totals)[None], 2, cols_of(before), tol=tol, hist_cap=4)
    fields_equal(got[0], frozen, "step 2 frozen")
    fields_equal(got[1], stopped, "step 2 stopped")
    fields_equal(got[2], column(**dict(live, s_norm=1.0)), "step 2 at tol")
    fields_equal(got[3], column(**dict(live, s_norm=0.75, x_step=1, converged=1, done=1, iterations=3, residual=0.75)), "step 2 half step")
    fields_equal(got[4], column(**dict(live, s_norm=np.nan)), "step 2 NaN")
    assert hist[3][3] == 0.75 and np.all(hist[:3] == FILL) and np.all(hist[4] == FILL)
    # step 3: omega = t.s / t.t, or the breakdown on either: x_step 1, ||s|| recorded
    live = dict(live, s_norm=1.0)
    before = [frozen, stopped] + [column(**live)] * 5
    ts, tt = [2.0, 2.0, 2.0, 0.0, 2.0, np.inf, 2.0], [4.0, 4.0, 4.0, 4.0, 0.0, 4.0, np.nan]
    got, hist = run_reduce(Blab, 7, np.stack([integer_partials(ts), integer_partials(tt)]), 3, cols_of(before), tol=tol, hist_cap=4)
    fields_equal(got[0], frozen, "step 3 frozen")
    fields_equal(got[1], stopped, "step 3 stopped")
    fields_equal(got[2], column(**dict(live, omega=0.5)), "step 3 usable")
    for j in (3, 4, 5, 6):
        fields_equal(got[j], column(**dict(live, omega=0.0, x_step=1, breakdown=2, done=1, iterations=3, residual=1.0)), ("step 3 unusable", j))
        assert hist[j][3] == 1.0
    assert np.all(hist[:3] == FILL)
    # step 4: ||r|| counted and recorded, then the strict test, then rho' (breakdown 3) or beta = (rho' / rho) (alpha / omega)
    live = dict(live, omega=0.5)
    before = [frozen, stopped] + [column(**live)] * 5
    rr, hr = [9.0, 9.0, 9.0, 1.0, 0.5625, 9.0, 9.0], [4.0, 4.0, 4.0, 4.0, 4.0, 0.0, -np.inf]
    parts = np.stack([integer_partials(rr), integer_partials(hr)])
    got, hist = run_reduce(Blab, 7, parts, 4, cols_of(before), tol=tol, hist_cap=4)
    after = dict(live, iterations=3)
    fields_equal(got[0], frozen, "step 4 frozen")
    fields_equal(got[1], stopped, "step 4 stopped")
    fields_equal(got[2], column(**dict(after, residual=3.0, beta=4.0, rho=4.0)), "step 4 goes on")
    fields_equal(got[3], column(**dict(after, residual=1.0, beta=4.0, rho=4.0)), "step 4 at tol")
    fields_equal(got[4], column(**dict(after, residual=0.75, converged=1, done=1)), "step 4 below tol")
    for j in (5, 6):
        fields_equal(got[j], column(**dict(after, residual=3.0, breakdown=3, done=1)), ("step 4 unusable rho'", j))
    assert np.all(hist[:2] == FILL) and hist[2][3] == 3.0 and hist[4][3] == 0.75 and np.all(hist[2:, :3] == FILL)
    # the history guard iterations < hist_cap: iteration 3 does not fit a history of 3
    got, hist = run_reduce(Blab, 7, parts, 4, cols_of(before), tol=tol, hist_cap=3)
    assert np.all(hist == FILL) and got[2]["iterations"] == 3 and got[2]["residual"] == 3.0
