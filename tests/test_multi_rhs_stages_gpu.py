"""The batched solver's kernels (csrc/spmm_kernels.hip, csrc/cg_multi.hip) one at a time, for every k = 1..8, through the LAB
build's spmv_amd_cg_multi_stage -- the launches spmv_amd_cg_solve_device_multi makes, on caller data. Element-wise results are
BIT-exact against the oracle's fma forms and the oracle's SpMV, column by column; the dot partials are BIT-equal to the numpy
restatement of block_partials (tests/multi_rhs_restatement.py) and, per column, the same bits whatever k is and whatever slot the
column sits in (compared with the k = 1 launch of that column); the reduction's totals are held to 1e-13 of sum|terms| against
math.fsum and must be bit-reproducible; the scalar step is read field by field on totals that are exactly representable. Every
output array lies between 16 sentinel doubles that must survive each call (Guarded, tests/test_pcg_stages_gpu.py), inputs must
come back unchanged, and a repeated call gives the same bits."""
import math

import numpy as np
import pytest

import matrices as M
import multi_rhs_restatement as R
from bitwise import same_bits
from test_multi_rhs_gpu import random_stencil
from test_pcg_stages_gpu import GUARD, SENTINEL, SUM_TOL, Guarded

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
SIZES = [1, 2, 255, 256, 257, 1000, 4097]          # a lone tail row, whole workgroups, a tail of 1 (workgroup = 256 rows)
COUNTS = [1, 255, 256, 257, 4096, 4097, 8193]      # the slice is 4096 partials: one slice, an exact one, a short last, three
GRIDS = [3, 65, 257, 513, 576, 641, 700]           # 65, 257, 513, 641: ONE live column in the last wave; 576: dead waves beside a
                                                   # full one; 3: inside one wave
COL = np.dtype([("rr_old", "f8"), ("pAp", "f8"), ("alpha", "f8"), ("beta", "f8"), ("b_norm", "f8"), ("residual", "f8"),
                ("active", "i4"), ("done", "i4"), ("iterations", "i4"), ("pad", "i4")])
assert COL.itemsize == 64


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


class Shifted(Guarded):
    """Guarded with the payload one double further into the allocation: 8- but not 16-byte aligned."""

    def __init__(self, Blab, values):
        self.B = Blab
        self.n = len(values)
        self.lead = GUARD + 1
        host = np.full(self.n + 2 * GUARD + 1, SENTINEL)
        host[self.lead:self.lead + self.n] = values
        self.dev = Blab.DeviceVector.from_host(host)
        self.ptr = self.dev.ptr + 8 * self.lead
        assert self.ptr % 16 == 8

    def read(self):
        host = self.dev.to_host()
        assert np.all(host[:self.lead] == SENTINEL) and np.all(host[self.lead + self.n:] == SENTINEL), "written outside the array"
        return host[self.lead:self.lead + self.n].copy()


def interleave(columns):
    """(k, n) columns -> [row * k + j]"""
    return np.ascontiguousarray(np.asarray(columns).T).ravel()


def columns_of(flat, k):
    return np.ascontiguousarray(flat.reshape(-1, k).T)


def records(k, **fields):
    c = np.zeros(k, dtype=COL)
    for name, v in fields.items():
        c[name] = v
    return c


def as_doubles(cols):
    return cols.view(np.float64).copy()


def as_records(doubles):
    return doubles.view(COL).copy()


# ---------------------------------------------------------------- the vector stages
def column_data(n, c):
    """The four vectors and the two scalars of column id c at size n: a column's data never depends on k or on its slot."""
    rng = np.random.default_rng(100 * n + c)
    b, ap, p, x = (rng.standard_normal(n) for _ in range(4))
    return b, ap, p, x, float(rng.uniform(0.25, 2.0)) * (-1.0) ** c, float(rng.uniform(0.25, 2.0))


def scenarios(k):
    """(name, slot of the special column or None, its active, its done): all live; one frozen column (active = 0) and one column
    converging in this iteration (active = 1, done = 1), each at slot 0, at slot 1 (the other half of slot 0's 16-byte pair) and at
    slot k - 1."""
    out = [("all live", None, 1, 0)]
    for slot in sorted({0, min(1, k - 1), k - 1}):
        out.append((f"frozen at {slot}", slot, 0, 0))
        out.append((f"done at {slot}", slot, 1, 1))
    return out


def vector_stage(Blab, stage, k, n, ids, cols):
    """One launch of `stage` on the columns `ids` (column id per slot) with the records `cols`; returns the arrays afterwards."""
    data = [column_data(n, c) for c in ids]
    count = (n + 255) // 256
    host = {"R": interleave([d[0] for d in data]), "AP": interleave([d[1] for d in data]), "P": interleave([d[2] for d in data]),
            "X": interleave([d[3] for d in data])}
    if stage == "init":
        host["P"] = np.full(n * k, np.nan)  # written, never read
    dev = {name: Guarded(Blab, v) for name, v in host.items()}
    dcols = Guarded(Blab, as_doubles(cols))
    dpart = Guarded(Blab, np.full(k * count, np.nan))
    a = Blab.CgMultiStageArgs(n=n, X=dev["X"].ptr, R=dev["R"].ptr, P=dev["P"].ptr, AP=dev["AP"].ptr, cols=dcols.ptr, partials=dpart.ptr)
    assert Blab.cg_multi_stage(stage, k, a) == 0
    assert a.count == count
    out = {name: columns_of(v.read(), k) for name, v in dev.items()}
    out["partials"] = dpart.read().reshape(k, count)
    assert same_bits(dcols.read(), as_doubles(cols)), "the column records are read only"
    for v in list(dev.values()) + [dcols, dpart]:
        v.free()
    return out, data


_alone = {}


def alone(Blab, stage, n, c, rec):
    """The partials of column id c in a k = 1 launch with the record `rec` (cached: the k = 1 launch of that column)."""
    key = (stage, n, c, rec.tobytes())
    if key not in _alone:
        out, _ = vector_stage(Blab, stage, 1, n, [c], np.array(rec, dtype=COL).reshape(1))
        _alone[key] = out["partials"][0]
    return _alone[key]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_init_stage(Blab, O, n, k):
    """R = b - Ap per column (fma(1, b, -Ap) and the oracle's fma(-1, Ap, b) round the same exact value once), P = R, and the
    partials of r.r."""
    for rot in (0, 3):
        ids = [(s + rot) % 8 for s in range(k)]
        out, data = vector_stage(Blab, "init", k, n, ids, records(k))
        for s, (b, ap, p, x, _, _) in enumerate(data):
            want = O.axpy(-1.0, ap, b)
            assert same_bits(out["R"][s], want) and same_bits(out["P"][s], want), (rot, s)
            assert same_bits(out["AP"][s], ap) and same_bits(out["X"][s], x), (rot, s)  # inputs untouched
            assert same_bits(out["partials"][s], R.block_partials_of(want * want, R.flat())), (rot, s)
            assert same_bits(out["partials"][s], alone(Blab, "init", n, ids[s], records(1)[0])), (rot, s)
        again, _ = vector_stage(Blab, "init", k, n, ids, records(k))
        assert all(same_bits(again[name], out[name]) for name in out), rot


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_update_r_stage(Blab, O, n, k):
    """r_j = fma(-alpha_j, Ap_j, r_j) for the columns with active set (done is not this kernel's business); a frozen column keeps
    its bits, next to a live one in the same 16-byte pair too; the partials are those of r.r of every column, frozen or not."""
    for i, (name, slot, active, done) in enumerate(scenarios(k)):
        ids = [(s + i) % 8 for s in range(k)]
        cols = records(k, active=1, rr_old=np.nan, pAp=np.nan, b_norm=np.nan, residual=np.nan)
        for s, c in enumerate(ids):
            cols[s]["alpha"], cols[s]["beta"] = column_data(n, c)[4], np.nan  # beta is not read
        if slot is not None:
            cols[slot]["active"], cols[slot]["done"] = active, done
        out, data = vector_stage(Blab, "update_r", k, n, ids, cols)
        for s, (r, ap, p, x, alpha, _) in enumerate(data):
            want = O.axpy(-alpha, ap, r) if cols[s]["active"] else r
            assert same_bits(out["R"][s], want), (name, s)
            assert same_bits(out["AP"][s], ap) and same_bits(out["P"][s], p) and same_bits(out["X"][s], x), (name, s)
            assert same_bits(out["partials"][s], R.block_partials_of(want * want, R.flat())), (name, s)
            assert same_bits(out["partials"][s], alone(Blab, "update_r", n, ids[s], cols[s])), (name, s)
        if i == 0:
            again, _ = vector_stage(Blab, "update_r", k, n, ids, cols)
            assert all(same_bits(again[key], out[key]) for key in out)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_update_xp_stage(Blab, O, n, k):
    """x_j = fma(alpha_j, p_j, x_j), then p_j = fma(beta_j, p_j, r_j). A frozen column (active = 0) keeps x and p bit for bit; a
    column that converged in this iteration (done = 1) gets the x update and keeps p."""
    for i, (name, slot, active, done) in enumerate(scenarios(k)):
        ids = [(s + i) % 8 for s in range(k)]
        cols = records(k, active=1, rr_old=np.nan, pAp=np.nan, b_norm=np.nan, residual=np.nan)
        for s, c in enumerate(ids):
            cols[s]["alpha"], cols[s]["beta"] = column_data(n, c)[4:6]
        if slot is not None:
            cols[slot]["active"], cols[slot]["done"] = active, done
        out, data = vector_stage(Blab, "update_xp", k, n, ids, cols)
        for s, (r, ap, p, x, alpha, beta) in enumerate(data):
            want_x = O.axpy(alpha, p, x) if cols[s]["active"] else x
            want_p = O.update_p(r, beta, p) if cols[s]["active"] and not cols[s]["done"] else p
            assert same_bits(out["X"][s], want_x), (name, s)
            assert same_bits(out["P"][s], want_p), (name, s)
            assert same_bits(out["R"][s], r) and same_bits(out["AP"][s], ap), (name, s)
        assert np.all(np.isnan(out["partials"])), name  # this stage writes no partials
        if i == 0:
            again, _ = vector_stage(Blab, "update_xp", k, n, ids, cols)
            assert all(same_bits(again[key], out[key]) for key in ("X", "P", "R", "AP"))


# ---------------------------------------------------------------- the reduce stage
def reduce_stage(Blab, k, partials, which, cols, tol=0.0, hist=None, hist_cap=0):
    """`partials` (k, count), `cols` k records; returns the records and the history buffer afterwards."""
    partials = np.ascontiguousarray(partials, dtype=np.float64)
    dpart, dcols = Guarded(Blab, partials.ravel()), Guarded(Blab, as_doubles(cols))
    dhist = Guarded(Blab, np.full(max(k * hist_cap, 2), SENTINEL) if hist is None else hist)
    a = Blab.CgMultiStageArgs(partials=dpart.ptr, count=partials.shape[1], which=which, tol=tol, cols=dcols.ptr, hist=dhist.ptr,
                              hist_cap=hist_cap)
    assert Blab.cg_multi_stage("reduce", k, a) == 0
    assert same_bits(dpart.read(), partials.ravel()), "the partials are read only"
    got, h = as_records(dcols.read()), dhist.read()
    for v in (dpart, dcols, dhist):
        v.free()
    return got, h


def partials_of(count, c):
    return np.random.default_rng(1000 * count + c).standard_normal(count)


def totals(Blab, k, partials):
    """The k totals as step 1 leaves them in pAp (every column live: rr_old = 1, so alpha = 1 / total)."""
    got, _ = reduce_stage(Blab, k, partials, 1, records(k, rr_old=1.0))
    assert np.all(got["active"] == 1) and same_bits(got["alpha"], 1.0 / got["pAp"])
    return got["pAp"].copy()


_alone_total = {}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("count", COUNTS)
def test_reduction_totals(Blab, count, k):
    for rot in (0, 5):
        ids = [(s + rot) % 8 for s in range(k)]
        partials = np.stack([partials_of(count, c) for c in ids])
        got = totals(Blab, k, partials)
        for s, c in enumerate(ids):
            want, mag = math.fsum(partials[s]), float(np.sum(np.abs(partials[s])))
            print(f"count={count} k={k} slot={s} column={c}: err {abs(got[s] - want) / mag:.2e} of sum|terms|")
            assert abs(got[s] - want) <= SUM_TOL * mag, (rot, s)
            if (count, c) not in _alone_total:
                _alone_total[(count, c)] = totals(Blab, 1, partials[s:s + 1])[0]
            assert same_bits(got[s], _alone_total[(count, c)]), (rot, s)  # the same bits whatever k and slot
        assert same_bits(totals(Blab, k, partials), got), rot          # fixed shape: the same bits again


def integer_partials(k, totals_wanted, count=5):
    """k rows of `count` integer-valued partials with the given totals (exact in any order of summation)."""
    p = np.zeros((k, count))
    for s, t in enumerate(totals_wanted):
        p[s, 1:] = np.arange(1, count) * (1 + s % 3)
        p[s, 0] = t - p[s, 1:].sum()
    return p


GARBAGE = dict(rr_old=7.0, pAp=7.0, alpha=7.0, beta=7.0, b_norm=7.0, residual=7.0, active=7, done=7, iterations=7, pad=7)


def check_records(got, want, what):
    for name in COL.names:
        if name != "pad":
            assert np.array_equal(got[name].view(np.uint64 if COL[name] == np.float64 else np.uint32),
                                  want[name].view(np.uint64 if COL[name] == np.float64 else np.uint32)), (what, name, got[name], want[name])


@pytest.mark.parametrize("k", KS)
def test_step_0_initial_scalars(Blab, k):
    """which = 0: every field reset from the total, h[0] written -- column j's history row starts at j * hist_cap."""
    squares = [float((s + 2) ** 2) for s in range(k)]  # b_norm = s + 2 exactly
    for cap in (1, 3):
        got, h = reduce_stage(Blab, k, integer_partials(k, squares), 0, records(k, **GARBAGE), hist_cap=cap)
        want = records(k, rr_old=squares, b_norm=np.sqrt(squares), residual=np.sqrt(squares))
        check_records(got, want, cap)
        want_h = np.full(max(k * cap, 2), SENTINEL)
        want_h[np.arange(k) * cap] = np.sqrt(squares)
        assert np.array_equal(h, want_h), cap


@pytest.mark.parametrize("k", KS)
def test_step_1_alpha_and_the_done_columns(Blab, k):
    """which = 1: active = !done; a live column gets pAp = total and alpha = rr_old / total (one IEEE division); a done column
    keeps pAp and alpha. Nothing else moves, the history is not touched."""
    for rot in range(2):
        done = np.array([(s + rot) % 2 for s in range(k)])
        p_ap = np.array([3.0 + 2 * s for s in range(k)]) * np.where(np.arange(k) % 3 == 2, -1.0, 1.0)  # a negative pAp is an ordinary value
        cols = records(k, rr_old=[1.5 + s for s in range(k)], pAp=9.0, alpha=0.125, beta=0.25, b_norm=8.0, residual=2.0, active=done,
                       done=done, iterations=[3 + s for s in range(k)])
        got, h = reduce_stage(Blab, k, integer_partials(k, p_ap), 1, cols, hist_cap=4)
        want = cols.copy()
        want["active"] = 1 - done
        live = done == 0
        want["pAp"][live] = p_ap[live]
        want["alpha"][live] = cols["rr_old"][live] / p_ap[live]
        check_records(got, want, rot)
        assert np.all(h == SENTINEL)


# the kinds of column step 2 meets, as (b_norm, iterations before, active): r.r = 16, so ||r|| = 4, and tol = 0.5, cap = 6
STEP2 = {
    "far": (1.0, 2, 1),                               # 4 / 1 = 4: goes on
    "equal": (8.0, 0, 1),                             # 4 / 8 == tol: the test is strict, goes on
    "converging": (float(np.nextafter(8.0, 9.0)), 1, 1),  # the next ratio below tol: converges
    "inactive": (1.0, 2, 0),                          # frozen: untouched
    "last entry": (1.0, 4, 1),                        # iterations + 1 == cap - 1: written
    "past the end": (1.0, 5, 1),                      # iterations + 1 == cap: nothing written
    "converging past the end": (64.0, 7, 1),
}


@pytest.mark.parametrize("k", KS)
def test_step_2_history_verdict_and_beta(Blab, k):
    kinds = list(STEP2)
    cap, tol, total = 6, 0.5, 16.0
    for rot in range(len(kinds)):
        mine = [kinds[(s + rot) % len(kinds)] for s in range(k)]
        cols = records(k, rr_old=[2.0 + s for s in range(k)], pAp=9.0, alpha=0.5, beta=0.25, residual=2.0,
                       b_norm=[STEP2[m][0] for m in mine], iterations=[STEP2[m][1] for m in mine], active=[STEP2[m][2] for m in mine])
        hist0 = np.arange(k * cap, dtype=np.float64) + 0.5  # every entry distinct: a write to the wrong row shows
        got, h = reduce_stage(Blab, k, integer_partials(k, [total] * k), 2, cols, tol=tol, hist=hist0, hist_cap=cap)
        want, want_h = cols.copy(), hist0.copy()
        for s, m in enumerate(mine):
            if not STEP2[m][2]:
                continue
            it = STEP2[m][1] + 1
            want[s]["iterations"], want[s]["residual"] = it, 4.0
            if it < cap:
                want_h[s * cap + it] = 4.0
            if np.float64(4.0) / np.float64(STEP2[m][0]) < tol:
                want[s]["done"] = 1
            else:
                want[s]["beta"] = np.float64(total) / cols[s]["rr_old"]
                want[s]["rr_old"] = total
        assert [bool(w["done"]) for w in want] == [m.startswith("converging") for m in mine]
        check_records(got, want, (rot, mine))
        assert np.array_equal(h, want_h), (rot, mine)  # and the sentinels behind the last row survived (Guarded)


# ---------------------------------------------------------------- the SpMM stage
VARIANTS = {"row-lds": ("stencil5-csr", "grid"), "row-direct": ("stencil5-csr", "grid"), "row-generic": ("stencil5-csr", "flat"),
            "csr": ("cusparse-csr", "flat")}
_systems = {}


def system(O, n):
    """Random stencil coefficients and 8 random columns on an n x n grid with the oracle's products (kept for the last two n)."""
    if n not in _systems:
        while len(_systems) >= 2:
            _systems.pop(next(iter(_systems)))
        e = random_stencil(O, n, 100 + n)
        rows = n * n
        rp, ci, va = O.build_csr(e, rows)
        X = np.random.default_rng(n).standard_normal((8, rows))
        want = {"stencil5-csr": np.stack([O.spmv_stencil5(rp, ci, va, X[j], n) for j in range(8)]),
                "cusparse-csr": np.stack([O.spmv_csr(rp, ci, va, X[j]) for j in range(8)])}
        _systems[n] = (e, rows, X, want)
    return _systems[n]


def spmm_stage(Blab, mode, k, dx, rows, partial_count, xcd_run=0, holder=Guarded):
    """One launch; returns Y (k, rows), the partials (k, count) or None, and a->count."""
    dy = holder(Blab, np.full(rows * k, np.nan))
    dpart = None if partial_count is None else Guarded(Blab, np.full(k * partial_count, np.nan))
    a = Blab.CgMultiStageArgs(mode=mode.encode(), X=dx.ptr, AP=dy.ptr, partials=None if dpart is None else dpart.ptr, xcd_run=xcd_run)
    assert Blab.cg_multi_stage("spmm", k, a) == 0
    Y = columns_of(dy.read(), k)
    parts = None if dpart is None else dpart.read().reshape(k, partial_count)
    dy.free()
    if dpart is not None:
        dpart.free()
    return Y, parts, a.count


def check_spmm(Blab, mode, layout, X, want, ks=KS, runs=(0,)):
    """Every k: Y with and without partials against `want`, the partials against the restatement and, per column id, against the
    first launch that held that column; on 8-byte-aligned vectors (even k: the 8-byte-access kernels) the same bits; `runs`:
    the XCD run lengths to repeat it all with."""
    rows = X.shape[1]
    count = R.block_count(rows, layout)
    first = {}
    for k in ks:
        ids = [(s + k) % 8 for s in range(k)]
        inter = interleave(X[ids])
        dx, dx8 = Guarded(Blab, inter), Shifted(Blab, inter)
        for run in runs:
            Y0, none, c0 = spmm_stage(Blab, mode, k, dx, rows, None, run)
            Y1, parts, c1 = spmm_stage(Blab, mode, k, dx, rows, count, run)
            Y2, parts8, c2 = spmm_stage(Blab, mode, k, dx8, rows, count, run, holder=Shifted)
            assert none is None and c0 == c1 == c2 == count, (k, run)
            for s, c in enumerate(ids):
                assert same_bits(Y0[s], want[c]) and same_bits(Y1[s], want[c]) and same_bits(Y2[s], want[c]), (k, run, s)
                if c not in first:
                    first[c] = parts[s].copy()
                    assert same_bits(first[c], R.block_partials_of(X[c] * want[c], layout)), (k, run, s)
                assert same_bits(parts[s], first[c]) and same_bits(parts8[s], first[c]), (k, run, s)
        Y1b, partsb, _ = spmm_stage(Blab, mode, k, dx, rows, count, runs[-1])
        assert same_bits(Y1b, Y1) and same_bits(partsb, parts), k   # a repeated call: the same bits
        assert same_bits(dx.read(), inter) and same_bits(dx8.read(), inter), k  # X is read only
        dx.free(), dx8.free()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", GRIDS)
def test_spmm_stage_stencil(Blab, O, n, variant):
    mode, kind = VARIANTS[variant]
    e, rows, X, want = system(O, n)
    Blab.lib().spmv_amd_reset_host_matrices()
    m = Blab.HostMatrix(e, rows, rows, n)
    op = Blab.Operator(mode)
    assert op.init(m) == 0
    try:
        if mode == "stencil5-csr":
            op.select_variant(variant)
            assert op.spmm_variant() == "spmm/stencil5-" + variant
        else:
            assert op.spmm_variant() == "spmm/csr"
        check_spmm(Blab, mode, R.grid(n) if kind == "grid" else R.flat(), X, want[mode])
    finally:
        if mode == "stencil5-csr":
            op.select_variant(None)
        op.free()
        Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.parametrize("n", [513, 641])
def test_spmm_stage_row_lds_xcd_runs(Blab, O, n):
    """The XCD-run remapping of row-lds (the product's plan takes it from n = 8000 on): runs of 3 and 5 do not divide the
    workgroup counts (1539, 1923), so the grid is padded and the padding returns early; Y and the partial bits are those of run 1,
    on 16- and on 8-byte-aligned vectors, and nothing is written outside Y or the partials."""
    e, rows, X, want = system(O, n)
    assert all(R.block_count(rows, R.grid(n)) % (8 * run) for run in (3, 5))
    Blab.lib().spmv_amd_reset_host_matrices()
    m = Blab.HostMatrix(e, rows, rows, n)
    op = Blab.Operator("stencil5-csr")
    assert op.init(m) == 0
    try:
        op.select_variant("row-lds")
        assert op.spmm_variant() == "spmm/stencil5-row-lds"
        check_spmm(Blab, "stencil5-csr", R.grid(n), X, want["stencil5-csr"], runs=(1, 3, 5))
    finally:
        op.select_variant(None)
        op.free()
        Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.parametrize("mode", ["stencil5-csr", "cusparse-csr"])
def test_spmm_stage_non_stencil_matrix(Blab, O, mode):
    """M.banded(3000, 7): the stencil operator's CSR loop and the CSR operator's spmm/csr, flat rows."""
    e, rows, cols, _ = M.banded(3000, 7)
    rp, ci, va = O.build_csr(e, rows)
    X = np.random.default_rng(7).standard_normal((8, cols))
    want = np.stack([O.spmv_csr(rp, ci, va, X[j]) for j in range(8)])
    Blab.lib().spmv_amd_reset_host_matrices()
    op = Blab.Operator(mode)
    assert op.init(Blab.HostMatrix(e, rows, cols, -1)) == 0
    try:
        assert op.spmm_variant() == ("spmm/stencil5-row-generic(csr-loop)" if mode == "stencil5-csr" else "spmm/csr")
        check_spmm(Blab, mode, R.flat(), X, want)
    finally:
        op.free()
        Blab.lib().spmv_amd_reset_host_matrices()
