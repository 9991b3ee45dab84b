"""The batched GCR solver's kernels (csrc/gcr_multi.hip) one at a time, for odd and even k and both kinds, through the LAB build's
spmv_amd_gcr_multi_stage -- the launches spmv_amd_gcr_solve_device_multi makes, on caller data. Element-wise results are BIT-exact
against the oracle's fma forms with i ascending; every partial set is BIT-equal to the restatement of block_partials
(tests/multi_rhs_restatement.py) computed from the column's own data -- so a column has the same bits whatever k is and whatever slot
it sits in; the reduction's totals are BIT-equal to reduce_multi, through one slice and through two (the ticket); every scalar step is
read field by field. The multidot runs at slots 1, chunk, chunk + 1 and 31, the orthogonalise kernel at slots 0, 1, chunk + 1 and 31,
n is no multiple of 256, z_in may BE R. A frozen column -- tried in slot 0, slot 1 (the other half of slot 0's 16-byte pair) and the
last slot -- is NaN-POISONED in every vector on entry: it must come back bit-identical, its partials must be 0.0 and no other column's
bits may change; with every column frozen the outputs keep their sentinel values. Every array lies between sentinel doubles that must
survive each call (Guarded)."""
import ctypes as C

import numpy as np
import pytest

import multi_rhs_restatement as M
import reduction_restatement as RR
from bitwise import same_bits
from test_multi_rhs_stages_gpu import columns_of, interleave
from test_pcg_stages_gpu import Guarded

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
SIZES = [1, 257, 513]  # a lone row, a tail of one row, three workgroups with a tail (workgroup = 256 rows)
KINDS = ["none", "jacobi"]
MAXR = 32
COL = np.dtype([("gamma", "f8", MAXR), ("beta", "f8", MAXR), ("alpha", "f8"), ("rho", "f8"), ("b_norm", "f8"), ("residual", "f8"),
                ("done", "i4"), ("iterations", "i4"), ("converged", "i4"), ("breakdown", "i4")])
SHADOW = np.dtype([("rz", "f8"), ("pAp", "f8"), ("alpha", "f8"), ("beta", "f8"), ("b_norm", "f8"), ("residual", "f8"), ("active", "i4"),
                   ("done", "i4"), ("iterations", "i4"), ("converged", "i4"), ("breakdown", "i4"), ("skip_update", "i4"), ("pad", "i4", 2)])
assert COL.itemsize == 560 and SHADOW.itemsize == 80
FILL = -7.25  # what an output array holds before the launch: a value no result has


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


def column_data(n, c, slot):
    """The vectors and scalars of column id c at size n: a column's data never depends on k or on its position."""
    rng = np.random.default_rng(100 * n + c)
    v = {name: rng.standard_normal(n) for name in ("X", "R", "AX", "ZIN", "ZS")}
    v["Q"] = rng.standard_normal((MAXR, n))[:slot + 1]
    v["Z"] = rng.standard_normal((MAXR, n))[:slot + 1]
    v["beta"] = rng.uniform(0.25, 2.0, MAXR) * np.where(np.arange(MAXR) % 2 == c % 2, -1.0, 1.0)
    v["alpha"] = float(rng.uniform(0.25, 2.0)) * (-1.0) ** c
    return v


def dinv_of(n):
    return np.random.default_rng(n).uniform(0.5, 2.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)


def scenarios(k):
    """Every column running; a frozen one at slot 0, slot 1 and the last slot; every column frozen."""
    out = [[False] * k]
    for s in sorted({0, min(1, k - 1), k - 1}):
        row = [False] * k
        row[s] = True
        out.append(row)
    out.append([True] * k)
    return out


def fma(O, a, u, c):
    return O.fma(np.full(len(u), float(a)), u, c)


def partials_of(prod):
    return M.block_partials_of(np.ascontiguousarray(prod, dtype=np.float64), M.flat())


def run_stage(Blab, stage, kind, k, n, slot, ids, frozen, alias=False):
    """One launch on the columns `ids`; frozen[s]: column s is done and all its vectors hold NaN. alias: z_in IS R. Returns the arrays
    afterwards per column, the partials (32, k, count) and the columns' data as they went in."""
    jac = kind == "jacobi"
    data = [column_data(n, c, slot) for c in ids]
    for d, f in zip(data, frozen):
        if f:
            for name in ("X", "R", "AX", "ZIN", "ZS"):
                d[name] = np.full(n, np.nan)
            d["Q"], d["Z"] = np.full((slot + 1, n), np.nan), np.full((slot + 1, n), np.nan)
    for d in data:
        if alias:
            d["ZIN"] = d["R"]
    dinv = dinv_of(n)
    count = (n + 255) // 256
    dev = {name: Guarded(Blab, interleave([d[name] for d in data])) for name in ("X", "R", "AX", "ZIN", "ZS")}
    dq = [Guarded(Blab, interleave([d["Q"][i] for d in data])) for i in range(slot + 1)]
    dz = [Guarded(Blab, interleave([d["Z"][i] for d in data])) for i in range(slot + 1)]
    cols = np.zeros(k, dtype=COL)
    for s, d in enumerate(data):
        cols[s]["beta"], cols[s]["alpha"], cols[s]["gamma"], cols[s]["b_norm"], cols[s]["done"] = d["beta"], d["alpha"], 1.5, 2.5, int(frozen[s])
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    ddinv = Guarded(Blab, dinv)
    dpart = Guarded(Blab, np.full(MAXR * k * count, FILL))
    Q = (C.c_void_p * MAXR)(*([q.ptr for q in dq] + [8] * (MAXR - slot - 1)))  # slots above `slot`: crooked pointers nobody may look at
    Z = (C.c_void_p * MAXR)(*([z.ptr for z in dz] + [8] * (MAXR - slot - 1)))
    a = Blab.GcrMultiStageArgs(n=n, X=dev["X"].ptr, R=dev["R"].ptr, AX=dev["AX"].ptr, z_in=dev["R"].ptr if alias else dev["ZIN"].ptr,
                               ZS=dev["ZS"].ptr if jac else None, Q=Q, Z=Z, slot=slot, dinv=ddinv.ptr if jac else None, cols=dcols.ptr,
                               partials=dpart.ptr)
    assert Blab.gcr_multi_stage(stage, kind, k, a) == 0
    assert a.count == count
    out = {name: columns_of(v.read(), k) for name, v in dev.items()}
    out["Q"] = [columns_of(q.read(), k) for q in dq]
    out["Z"] = [columns_of(z.read(), k) for z in dz]
    out["partials"] = dpart.read().reshape(MAXR, k, count)
    assert same_bits(dcols.read(), cols.view(np.float64)), "the column records are read only"
    assert same_bits(ddinv.read(), dinv), "dinv is read only"
    for v in list(dev.values()) + dq + dz + [dcols, ddinv, dpart]:
        v.free()
    return out, data, dinv


def check_unchanged(out, data, s, label, but=()):
    """Everything of column s came back as it went in, except the names in `but` ("Q3": slot 3 of Q)."""
    for name in ("X", "R", "AX", "ZIN", "ZS"):
        if name not in but:
            assert same_bits(out[name][s], data[s][name]), (label, name, "changed")
    for name in ("Q", "Z"):
        for i in range(len(out[name])):
            if f"{name}{i}" not in but:
                assert same_bits(out[name][i][s], data[s][name][i]), (label, name, i, "changed")


def check_partials(out, s, values, label):
    """values[v]: the column's products per row of value v, or 0.0 for a frozen column; every value behind them is untouched."""
    for v in range(MAXR):
        got = out["partials"][v][s]
        if v >= len(values):
            assert np.all(got == FILL), (label, v, "written")
        else:
            n = len(out["R"][s])
            assert same_bits(got, partials_of(np.broadcast_to(np.asarray(values[v], dtype=np.float64), (n,)))), (label, v)


def ids_for(k, rot):
    return [(s + rot) % 8 for s in range(k)]


# ---------------------------------------------------------------- init
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, O, n, kind):
    for k in KS:
        out, data, dinv = run_stage(Blab, "init", kind, k, n, 0, ids_for(k, k), [False] * k)
        for s in range(k):
            label = (n, kind, k, s)
            r = O.axpy(-1.0, data[s]["AX"], data[s]["R"])  # fma(1.0, b, -1.0 * Ax0): one rounding of b - Ax0
            assert same_bits(out["R"][s], r), label
            if kind == "jacobi":
                assert same_bits(out["ZS"][s], dinv * r), label
            check_unchanged(out, data, s, label, but=("R", "ZS") if kind == "jacobi" else ("R",))
            check_partials(out, s, [r * r], label)


# ---------------------------------------------------------------- multidot
@pytest.mark.parametrize("slot", [1, 4, 5, 31])
@pytest.mark.parametrize("n", SIZES)
def test_multidot_stage(Blab, n, slot):
    """Slots 1, chunk, chunk + 1 and 31 (kDotChunk = 4): value i of a running column is the partials of Q_i . Q_slot."""
    assert Blab.GCR_MULTI_DOT_CHUNK == 4
    for k in (KS if slot < 31 else (1, 3, 8)):
        for frozen in scenarios(k):
            out, data, _ = run_stage(Blab, "multidot", None, k, n, slot, ids_for(k, slot), frozen)
            for s in range(k):
                label = (n, slot, k, frozen, s)
                check_unchanged(out, data, s, label)
                if all(frozen):
                    check_partials(out, s, [], label)
                else:
                    check_partials(out, s, [0.0 if frozen[s] else data[s]["Q"][i] * data[s]["Q"][slot] for i in range(slot)], label)


# ---------------------------------------------------------------- orthogonalise
@pytest.mark.parametrize("alias", [False, True], ids=["z_in", "z_in-is-R"])
@pytest.mark.parametrize("slot", [0, 1, 3, 31])
@pytest.mark.parametrize("n", SIZES)
def test_orthogonalise_stage(Blab, O, n, slot, alias):
    """Slots 0, 1, chunk + 1 and 31 (kOrthChunk = 2): i ascending, q in place, z out of place into Z_slot (slot 0: z only moves); the
    partials of q.q and r.q; z_in aliased to R gives the same bits as a copy would."""
    assert Blab.GCR_MULTI_ORTH_CHUNK == 2
    for k in (KS if slot < 31 else (1, 3, 8)):
        for frozen in scenarios(k):
            out, data, _ = run_stage(Blab, "orthogonalise", None, k, n, slot, ids_for(k, slot + 1), frozen, alias=alias)
            for s in range(k):
                label = (n, slot, k, frozen, s, alias)
                if frozen[s]:
                    check_unchanged(out, data, s, label)
                    check_partials(out, s, [] if all(frozen) else [0.0, 0.0], label)
                    continue
                d = data[s]
                q, z = d["Q"][slot], d["ZIN"]
                for i in range(slot):
                    q = fma(O, -d["beta"][i], d["Q"][i], q)
                    z = fma(O, -d["beta"][i], d["Z"][i], z)
                assert same_bits(out["Q"][slot][s], q) and same_bits(out["Z"][slot][s], z), label
                check_unchanged(out, data, s, label, but=(f"Q{slot}", f"Z{slot}"))
                check_partials(out, s, [q * q, d["R"] * q], label)


# ---------------------------------------------------------------- update_xr
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xr_stage(Blab, O, n, kind):
    for k in KS:
        for slot in (0, 5):
            for frozen in scenarios(k):
                out, data, dinv = run_stage(Blab, "update_xr", kind, k, n, slot, ids_for(k, 3), frozen)
                for s in range(k):
                    label = (n, kind, k, slot, frozen, s)
                    if frozen[s]:
                        check_unchanged(out, data, s, label)
                        check_partials(out, s, [] if all(frozen) else [0.0], label)
                        continue
                    d = data[s]
                    x = fma(O, d["alpha"], d["Z"][slot], d["X"])
                    r = fma(O, -d["alpha"], d["Q"][slot], d["R"])
                    assert same_bits(out["X"][s], x) and same_bits(out["R"][s], r), label
                    if kind == "jacobi":
                        assert same_bits(out["ZS"][s], dinv * r), label
                    check_unchanged(out, data, s, label, but=("X", "R", "ZS") if kind == "jacobi" else ("X", "R"))
                    check_partials(out, s, [r * r], label)


# ---------------------------------------------------------------- reduce
def run_reduce(Blab, k, count, which, slot, cols, partials, tol=1e-3, hist_cap=6):
    dpart = Guarded(Blab, partials.ravel())
    dcols = Guarded(Blab, cols.view(np.float64).copy())
    shadow = np.zeros(k, dtype=SHADOW)
    shadow["done"], shadow["rz"], shadow["active"] = 7, 3.25, 5
    dshadow = Guarded(Blab, shadow.view(np.float64).copy())
    dhist = Guarded(Blab, np.full(k * hist_cap, FILL))
    a = Blab.GcrMultiStageArgs(slot=slot, cols=dcols.ptr, shadow=dshadow.ptr, partials=dpart.ptr, count=count, which=which, tol=tol, hist=dhist.ptr,
                               hist_cap=hist_cap)
    assert Blab.gcr_multi_stage("reduce", None, k, a) == 0
    assert same_bits(dpart.read(), partials.ravel()), "the partials are read only"
    got = dcols.read().view(COL)
    sh = dshadow.read().view(SHADOW)
    hist = dhist.read().reshape(k, hist_cap)
    for v in (dpart, dcols, dshadow, dhist):
        v.free()
    return got, sh, hist, shadow


@pytest.mark.parametrize("count", [1, 4095, 4097])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_reduce_stage_and_every_scalar_step(Blab, k, count):
    """One slice (count <= 4096) and two (4097: the slice sums are published and the column's last ticket sums them), twice in a row on
    the same data. Step 0 resets the record; step 1 divides the `slot` sums by the gammas; step 2 takes
    alpha = rho / gamma or ends the column (gamma first); step 3 records ||r|| and tests it strictly. A column that is done keeps
    every bit of its record and its history; the shadow record's `done` follows, its other fields stay."""
    rng = np.random.default_rng(count + k)
    slot = 5
    partials = rng.standard_normal((MAXR, k, count))
    partials[0] = np.abs(partials[0])  # value 0 is a sum of squares wherever a step takes its root
    totals = np.array([[RR.reduce_multi(partials[v][s]) for s in range(k)] for v in range(MAXR)])

    def fresh(done_at=None):
        c = np.zeros(k, dtype=COL)
        c["gamma"], c["beta"] = rng.uniform(0.5, 2.0, (k, MAXR)), 9.5
        c["alpha"], c["rho"], c["b_norm"], c["residual"], c["iterations"] = 0.75, 1.25, 4.0, 3.5, 2
        if done_at is not None:
            c[done_at]["done"], c[done_at]["converged"] = 1, 1
        return c

    for frozen in (None, 0, k - 1):
        for which in (0, 1, 2, 3):
            cols = fresh(frozen)
            for _ in range(2):
                got, sh, hist, shadow = run_reduce(Blab, k, count, which, slot, cols, partials, tol=1e-3)
            for s in range(k):
                label = (k, count, which, frozen, s)
                c, g = cols[s], got[s]
                assert sh[s]["rz"] == 3.25 and sh[s]["active"] == 5, label
                if which == 0:
                    b_norm = np.sqrt(totals[0][s])
                    assert np.all(g["gamma"] == 0.0) and np.all(g["beta"] == 0.0) and g["alpha"] == 0.0 and g["rho"] == 0.0, label
                    assert g["b_norm"] == b_norm and g["residual"] == b_norm and hist[s][0] == b_norm and np.all(hist[s][1:] == FILL), label
                    assert (g["done"], g["iterations"], g["converged"], g["breakdown"], sh[s]["done"]) == (0, 0, 0, 0, 0), label
                    continue
                if frozen == s:
                    assert same_bits(got[s:s + 1].view(np.float64), cols[s:s + 1].view(np.float64)) and np.all(hist[s] == FILL), label
                    assert sh[s]["done"] == 7, label  # not even the shadow is written: it holds the column's `done` since the freeze
                    continue
                assert sh[s]["done"] == g["done"], label
                if which == 1:
                    want = c["beta"].copy()
                    want[:slot] = totals[:slot, s] / c["gamma"][:slot]
                    assert same_bits(g["beta"], want) and same_bits(g["gamma"], c["gamma"]) and g["done"] == 0 and np.all(hist[s] == FILL), label
                elif which == 2:
                    want = c["gamma"].copy()
                    want[slot] = totals[0][s]
                    assert same_bits(g["gamma"], want) and g["rho"] == totals[1][s] and g["alpha"] == totals[1][s] / totals[0][s], label
                    assert (g["done"], g["iterations"], g["breakdown"]) == (0, 2, 0) and np.all(hist[s] == FILL), label
                else:
                    res = np.sqrt(totals[0][s])
                    conv = int(res / c["b_norm"] < 1e-3)
                    assert g["residual"] == res and g["iterations"] == 3 and hist[s][3] == res and (g["converged"], g["done"]) == (conv, conv), label


def test_the_breakdowns_and_the_strict_test(Blab):
    """Totals that are exactly representable (count 1): gamma = 0, gamma = inf and rho = 0 end the column with the iteration counted and
    the UNCHANGED residual recorded; ||r|| / ||r0|| == tol does not converge, a norm just below does."""
    k = 3
    for which, values, want in ((2, [(0.0, 1.0), (np.inf, 2.0), (4.0, 0.0)], [(1, 1), (1, 1), (2, 1)]),
                                (2, [(4.0, np.nan), (4.0, 2.0), (np.nan, 0.0)], [(2, 1), (0, 0), (1, 1)]),
                                (3, [(4.0, 0.0), (3.9990234375, 0.0), (16.0, 0.0)], [(0, 0), (0, 1), (0, 0)])):
        partials = np.zeros((MAXR, k, 1))
        for s, (v0, v1) in enumerate(values):
            partials[0][s][0], partials[1][s][0] = v0, v1
        cols = np.zeros(k, dtype=COL)
        cols["b_norm"], cols["residual"], cols["iterations"], cols["alpha"] = 4.0, 3.5, 2, 0.75
        got, sh, hist, _ = run_reduce(Blab, k, 1, which, 1, cols, partials, tol=0.5)
        for s, (breakdown, done) in enumerate(want):
            g = got[s]
            assert (g["breakdown"], g["done"], sh[s]["done"]) == (breakdown, done, done), (which, s, g)
            if which == 2 and done:
                assert g["alpha"] == 0.0 and g["iterations"] == 3 and g["residual"] == 3.5 and hist[s][3] == 3.5 and g["converged"] == 0, (which, s)
                assert same_bits(g["gamma"], cols[s]["gamma"]), (which, s)
            if which == 2 and not done:
                assert g["alpha"] == 0.5 and g["gamma"][1] == 4.0 and g["iterations"] == 2, (which, s)
            if which == 3:
                assert g["converged"] == done and g["iterations"] == 3 and g["residual"] == np.sqrt(values[s][0]), (which, s)
