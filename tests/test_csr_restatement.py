"""The restatement of the general CSR kernels (tests/csr_restatement.py) on the CPU: its geometry at the edges of the rule, the chunk
walk of csr/adaptive on the table whose every block is one scenario, its sums against exact sums (an a-priori bound, not a measured
one), against the sequential sum where they must agree and where they must not, under poisoned inputs, and the fused partials against
the restatements they have to coincide with."""
import math
import re

import numpy as np
import pytest

import csr_restatement as CR
import matrices as M
import poison as P
import reduction_restatement as R
from bitwise import bits, same_bits


# ---------------------------------------------------------------- geometry
def test_stream_geometry_at_the_edges_of_its_rule():
    g = CR.stream_geometry
    assert g(1000, 1000) == (256, 4)       # a mean of exactly 1: 921 rows would fill the strip, one row per thread at most
    assert g(1000, 500) == (256, 4)        # below 1: the mean counts as 1
    assert g(1000, 0) == (256, 4)
    assert g(0, 0) == (256, 0)             # no rows: no blocks
    assert g(1, 5) == (176, 1)             # 184 -> 176
    assert g(257, 257) == (256, 2)
    # the cap: 921.6 / 3.6 = 256 exactly (3.6 is 4 x the double 0.9)
    assert g(1000, 3599) == (256, 4) and g(1000, 3600) == (256, 4)
    assert g(1000, 3601) == (240, 5)       # 255 -> 240
    # the floor: 921.6 / 57.6 = 16 exactly; 17 and 15 both end at 16, by the rounding and by the floor
    assert g(1000, 57600) == (16, 63) and g(1000, 57599) == (16, 63) and g(1000, 57601) == (16, 63)
    assert g(1000, 54000) == (16, 63)      # 17 -> 16
    assert g(1000, 1000000) == (16, 63)    # 0 -> 16
    # & ~15 rounds down: 153 -> 144, 31 -> 16, 32 stays
    assert g(1000, 6000) == (144, 7)
    assert g(1000, 28800) == (32, 32) and g(1000, 28801) == (16, 63)
    t = CR.adaptive_table()
    assert g(145, 25169) == (16, 10) and (len(t.rp) - 1, int(t.rp[-1])) == (145, 25169)


def test_auto_variant_at_its_two_thresholds():
    assert CR.auto_variant(100, 19200, 300) == "stream"       # a mean of exactly 192 is not above it
    assert CR.auto_variant(100, 19201, 300) == "wavefront"
    assert CR.auto_variant(100, 19201, 5000) == "wavefront"   # the mean is asked first
    assert CR.auto_variant(100, 5000, 1024) == "stream"       # a row of exactly one strip fits
    assert CR.auto_variant(100, 5000, 1025) == "adaptive"
    assert CR.auto_variant(0, 0, 0) == "stream"
    t = CR.adaptive_table()
    assert CR.variant_of(t.rp, None) == "adaptive" and CR.variant_of(t.rp, "csr/wavefront") == "wavefront"


# ---------------------------------------------------------------- the table
@pytest.fixture(scope="module")
def table():
    t = CR.adaptive_table()
    y, events = CR.adaptive_row_sums(t.rp, t.ci, t.va, t.x)
    return t, y, events


def test_the_table_is_what_it_says(table):
    t, _, _ = table
    assert len(t.x) == CR.TABLE_COLS == 6000 and abs(25169 / 145 - 173.6) < 0.05
    lengths = np.diff(t.rp)
    assert lengths.tolist() == [n for block, _, _ in CR.TABLE_BLOCKS for n in block]
    for r in range(145):  # sorted, distinct columns
        assert np.all(np.diff(t.ci[t.rp[r]:t.rp[r + 1]]) > 0), r
    assert np.all((np.abs(t.va) >= 0.25) & (np.abs(t.va) < 3.0))
    reserved = (t.ci < CR.RESERVED) | (t.ci >= CR.TABLE_COLS - CR.RESERVED)
    used = t.ci[reserved]
    assert len(used) == len(set(used.tolist())) and sorted(used.tolist()) == t.reserved.tolist()
    assert np.isinf(t.x_poisoned[0]) and np.isinf(t.x_poisoned[-1])  # what a dead slot gathering x[0] or a clamped index would meet
    assert np.all(np.isinf(t.x_poisoned[t.reserved])) and same_bits(np.delete(t.x_poisoned, t.reserved), np.delete(t.x, t.reserved))
    nonempty = np.flatnonzero(lengths > 0)
    for r in CR.TABLE_LONG_ROWS:
        front, behind = nonempty[nonempty < r], nonempty[nonempty > r]
        if len(front):
            assert t.ci[t.rp[front[-1] + 1] - 1] >= CR.TABLE_COLS - CR.RESERVED, r
        if len(behind):
            assert t.ci[t.rp[behind[0]]] < CR.RESERVED, r
    first, last = np.zeros(len(t.ci), dtype=bool), np.zeros(len(t.ci), dtype=bool)
    first[t.rp[:-1][lengths > 0]] = True
    last[t.rp[1:][lengths > 0] - 1] = True
    assert np.all(t.ci[reserved & first & ~last] < CR.RESERVED) and np.all(t.ci[reserved & last & ~first] >= CR.TABLE_COLS - CR.RESERVED)
    assert not np.any(reserved & ~first & ~last)


def test_events_are_the_chunk_walk_the_table_was_made_for(table):
    t, _, events = table
    per_block, blocks = CR.stream_geometry(145, int(t.rp[-1]))
    assert per_block == 16 and blocks == len(events) == 10
    assert events == [want for _, want, _ in CR.TABLE_BLOCKS]
    with_v, owners = set(), set()
    for g, ev in enumerate(events):
        for thread in re.findall(r"V(\d+)", ev):
            with_v.add(g * per_block + int(thread))
            owners.add(int(thread))
    assert sorted(with_v) == list(CR.TABLE_LONG_ROWS)
    assert owners >= {0, 1, 2, 4, 15}
    assert CR.auto_variant(145, int(t.rp[-1]), int(np.diff(t.rp).max())) == "adaptive"


# ---------------------------------------------------------------- against exact sums
def exact_row_sums(rp, ci, va, x):
    """math.fsum of the exactly formed products: v x = p + e with p the rounded product and e = fma(v, x, -p) (no overflow or
    underflow at these magnitudes). Returns the sums and sum |v x| per row."""
    from oracle import oracle as O

    xg = np.asarray(x)[ci]
    p = va * xg
    e = O.fma(va, xg, -p)
    exact = np.array([math.fsum(np.concatenate([p[a:b], e[a:b]])) for a, b in zip(rp[:-1], rp[1:])])
    mass = np.array([math.fsum(np.abs(p[a:b])) for a, b in zip(rp[:-1], rp[1:])])
    return exact, mass


def long_row_matrix(O):
    """The matrix of tests/test_spmv_gpu.py::test_csr_operator: rows 0, 1 and 137 of 3500 / 2900 / 2900 entries among short and empty ones"""
    e, r, c = M.random_sparse(300, 6000, lambda row, rng: (3500 if row == 0 else 2900) if row in (0, 1, 137) else (0 if row % 11 == 0 else int(rng.integers(1, 9))), seed=12)
    return O.build_csr(e, r) + (np.random.default_rng(6).standard_normal(c),)


def banded_matrix(O):
    e, r, c, _ = M.banded(3000, 160, diagonal=12.0)
    return O.build_csr(e, r) + (np.random.default_rng(11).standard_normal(c),)


@pytest.mark.parametrize("name", ["table", "long rows", "banded"])
def test_row_sums_within_the_a_priori_bound_of_an_exact_sum(O, name):
    """|y - exact| <= (L + 1) 2^-52 sum |v x| for a row of L entries: what any order of L fma or add steps keeps (each step's error
    is at most 2^-53 of a partial sum bounded by sum |v x| (1 + ...)), with a factor of two to spare."""
    if name == "table":
        t = CR.adaptive_table()
        rp, ci, va, x = t.rp, t.ci, t.va, t.x
    else:
        rp, ci, va, x = long_row_matrix(O) if name == "long rows" else banded_matrix(O)
    exact, mass = exact_row_sums(rp, ci, va, x)
    bound = (np.diff(rp) + 1) * 2.0 ** -52 * mass
    for what, y in (("adaptive", CR.adaptive_row_sums(rp, ci, va, x)[0]), ("wavefront", CR.wavefront_row_sums(rp, ci, va, x)),
                    ("sequential", O.spmv_csr(rp, ci, va, x))):
        err = np.abs(y - exact)
        print(name, what, "max |y - exact| / sum|v x| =", float(np.max(err / np.maximum(mass, 1e-300))))
        assert np.all(err <= bound), (name, what, int(np.argmax(err - bound)))
        assert same_bits(y[np.diff(rp) == 0], np.zeros(int((np.diff(rp) == 0).sum()))), (name, what)  # an empty row is +0.0


@pytest.mark.parametrize("name", ["table", "long rows", "banded"])
def test_integer_valued_data_is_exact_under_either_order(O, name):
    if name == "table":
        t = CR.adaptive_table()
        rp, ci, va = t.rp, t.ci, t.va
        cols = CR.TABLE_COLS
    else:
        rp, ci, va, x = long_row_matrix(O) if name == "long rows" else banded_matrix(O)
        cols = len(x)
    rng = np.random.default_rng(5)
    vi, xi = np.round(8.0 * va), np.round(8.0 * rng.standard_normal(cols))
    want = O.spmv_csr(rp, ci, vi, xi)
    assert np.any(want != 0.0)
    assert same_bits(CR.adaptive_row_sums(rp, ci, vi, xi)[0], want)
    assert same_bits(CR.wavefront_row_sums(rp, ci, vi, xi), want)


def test_the_tree_variants_differ_from_the_sequential_sum_where_they_should(O, table):
    t, y, _ = table
    seq = O.spmv_csr(t.rp, t.ci, t.va, t.x)
    long_rows = np.array(CR.TABLE_LONG_ROWS)
    others = np.setdiff1d(np.arange(145), long_rows)
    assert same_bits(y[others], seq[others])           # a row no flush reaches keeps the sequential sum, whatever its chunks were
    differs = bits(y[long_rows]) != bits(seq[long_rows])
    assert differs.sum() >= len(long_rows) // 2, differs  # thousands of entries in another order: equal bits are the exception
    # row 47, the 65-entry row: its last product goes through vacc, the trees and sum += t -- one rounding more than fma(v, x, sum);
    # whether that shows in the last bit depends on the data, so it is only held to the bound (the test above)
    w = CR.wavefront_row_sums(t.rp, t.ci, t.va, t.x)
    short = np.diff(t.rp) <= 1
    assert same_bits(w[short], seq[short])             # one entry: lane 0 alone, the tree adds +0.0
    assert (bits(w[~short]) != bits(seq[~short])).sum() >= 20


def test_rows_of_the_other_long_row_matrix(O):
    """The matrix the suite had: rows 0 and 1 share block 0, row 137 sits in block 8 (per_block 16 at a mean of 34)."""
    rp, ci, va, x = long_row_matrix(O)
    per_block, blocks = CR.stream_geometry(300, int(rp[-1]))
    assert (per_block, blocks) == (16, 19)
    y, events = CR.adaptive_row_sums(rp, ci, va, x)
    assert events[0].split()[:2] == ["V0", "V0"] and "F0" in events[0] and "V1" in events[0] and "F1" in events[0]
    assert "V9" in events[8] and all(ev.startswith("single:") for g, ev in enumerate(events) if g not in (0, 8))
    seq = O.spmv_csr(rp, ci, va, x)
    rest = np.setdiff1d(np.arange(300), [0, 1, 137])
    assert same_bits(y[rest], seq[rest])


def test_poisoned_x_reaches_exactly_the_rows_that_hold_it(O, table):
    t, y, _ = table
    with np.errstate(invalid="ignore"):
        yp, events = CR.adaptive_row_sums(t.rp, t.ci, t.va, t.x_poisoned)
        wp = CR.wavefront_row_sums(t.rp, t.ci, t.va, t.x_poisoned)
    seq = O.spmv_csr(t.rp, t.ci, t.va, t.x_poisoned)
    hit = P.poisoned_rows(t.rp, t.ci, t.reserved, [])
    assert 10 <= len(hit) <= 2 * len(CR.TABLE_LONG_ROWS)
    for got in (yp, wp, seq):
        assert np.flatnonzero(~np.isfinite(got)).tolist() == hit.tolist()
    clean = np.setdiff1d(np.arange(145), hit)
    assert same_bits(yp[clean], y[clean]) and events == [want for _, want, _ in CR.TABLE_BLOCKS]
    assert len(np.intersect1d(clean, CR.TABLE_LONG_ROWS)) >= 4  # long rows that stay finite next to poisoned neighbours


# ---------------------------------------------------------------- partials
def test_block_partials_coincide_with_the_restatements_they_must(O):
    rng = np.random.default_rng(77)
    for rows in (1, 255, 256, 257, 1000):
        x, s = rng.standard_normal(rows), rng.standard_normal(rows)
        assert same_bits(CR.stream_block_partials(x, s, 256), R.ell_partials(x, s)), rows
    # per_block 16: a slot is the tree over the 16 live lanes of wave 0, then + 0.0 three times
    rows = 145
    x, s = rng.standard_normal(rows), rng.standard_normal(rows)
    got = CR.stream_block_partials(x, s, 16)
    assert len(got) == 10
    for g in range(10):
        term = np.zeros(64)
        live = x[16 * g:16 * g + 16] * s[16 * g:16 * g + 16]
        term[:len(live)] = live
        assert same_bits(got[g], ((R.wave_tree(term) + 0.0) + 0.0) + 0.0), g
    # a product of -0.0 stays -0.0 in its lane, and a block of nothing but such products sums to -0.0 + 0.0 ... = +0.0 only through
    # the dead lanes: 16 live lanes of -0.0 in a wave of 64 give +0.0, a full block of 256 gives -0.0
    assert same_bits(CR.stream_block_partials(np.full(16, -1.0), np.zeros(16), 16), [0.0])
    assert same_bits(CR.stream_block_partials(np.full(256, -1.0), np.zeros(256), 256), [-0.0])
    # x may be longer than s (a square operator's x is indexed by the row)
    assert same_bits(CR.stream_block_partials(np.ones(20), np.ones(16), 16), [16.0])


def test_the_arrow_matrices_place_their_hubs_where_the_gpu_tests_need_them(O):
    for n, want in zip(CR.ARROW_SIZES, (144, 256)):
        a = CR.arrow(n)
        assert CR.stream_geometry(n, len(a.ci)) == (want, a.blocks) and a.per_block == want
        threads = [h % a.per_block for h in a.hubs]
        assert len(a.hubs) == 3 and a.hubs[-1] == n - 1
        assert 0 in threads and any(64 <= t < 128 for t in threads) and any(t >= 128 for t in threads)
        assert any(t == min(a.per_block, n - (h // a.per_block) * a.per_block) - 1 for t, h in zip(threads, a.hubs))
        lengths = np.diff(a.rp)
        assert sorted(np.flatnonzero(lengths > CR.CAP).tolist()) == list(a.hubs) and lengths[list(a.hubs)].min() >= CR.ARROW_SPOKES
        assert CR.variant_of(a.rp, None) == "adaptive"
        # symmetric bit for bit, diagonally dominant
        rows = P.row_of_entry(a.rp)
        fwd = dict(zip(zip(rows.tolist(), a.ci.tolist()), a.va.tolist()))
        assert all(fwd[(c, r)] == v for (r, c), v in fwd.items())
        off = np.bincount(rows, weights=np.where(rows == a.ci, 0.0, np.abs(a.va)), minlength=n)
        assert np.all(a.va[rows == a.ci] > off)
        _, events = CR.adaptive_row_sums(a.rp, a.ci, a.va, np.ones(n))
        owners = {int(t) for ev in events for t in re.findall(r"V(\d+)", ev)}
        assert owners == set(threads), (n, owners, threads)


def test_sums_worked_out_by_hand_show_the_order(O):
    """csr_restatement.hand_made: integers around 2^53, every expected value from its docstring and none from the code under test."""
    rp, ci, va, cols, want = CR.hand_made()
    assert CR.stream_geometry(17, len(ci)) == (16, 2)
    x = np.ones(cols)
    y, events = CR.adaptive_row_sums(rp, ci, va, x)
    assert events == ["S V1 F1 S", "single:65"]
    w = CR.wavefront_row_sums(rp, ci, va, x)
    seq = O.spmv_csr(rp, ci, va, x)
    got = {"adaptive": y, "wavefront": w, "stream": seq, "row-scalar": seq}
    for variant, rows in want.items():
        for row, value in rows.items():
            assert same_bits(got[variant][row], value), (variant, row, got[variant][row] - 2.0 ** 53)
    for v in (y, w, seq):
        assert same_bits(v[0], 0.0) and same_bits(v[2:16], np.full(14, 3.0))


def test_the_square_table_keeps_the_scenarios_of_blocks_0_to_8(O):
    rp, ci, va = CR.table_square()
    t = CR.adaptive_table()
    n = len(rp) - 1
    assert n == CR.TABLE_COLS and CR.stream_geometry(n, len(ci)) == (16, 375) and CR.variant_of(rp, None) == "adaptive"
    assert same_bits(va[:len(t.va)], t.va) and np.array_equal(ci[:len(t.ci)], t.ci) and np.array_equal(rp[:146], t.rp)
    assert np.all(np.diff(ci.astype(np.int64))[np.diff(P.row_of_entry(rp)) == 0] > 0)  # every row sorted, distinct columns
    assert ci[len(t.ci):].min() >= CR.RESERVED and ci.max() < CR.TABLE_COLS - CR.RESERVED + CR.RESERVED
    x = np.random.default_rng(1).standard_normal(n)
    y, events = CR.adaptive_row_sums(rp, ci, va, x)
    assert events[:9] == [want for _, want, _ in CR.TABLE_BLOCKS[:9]] and events[9] == "V0 V0 F0 S"
    assert events[10:] == ["single:960"] * 365
    seq = O.spmv_csr(rp, ci, va, x)
    rest = np.setdiff1d(np.arange(n), CR.TABLE_LONG_ROWS)
    assert same_bits(y[rest], seq[rest]) and not same_bits(y, seq)


def test_a_whole_restated_solve_converges_like_a_solve(O):
    """cg_restatement.solve on csr_restatement.system, the system tests/test_csr_gpu.py solves: under tolerance 0 the four variants
    run their 8 iterations, their first residuals agree to rounding (they differ in summation order only) and no two histories are
    equal in bits, so a solve held to one variant's restatement cannot pass on another's."""
    import cg_restatement as CG

    a = CR.arrow(3000)
    rng = np.random.default_rng(3000)
    b, x0 = rng.standard_normal(a.n), 0.1 * rng.standard_normal(a.n)
    runs = {v: CG.solve(CR.system(O, a.rp, a.ci, a.va, v), b, x0, 8, 0.0) for v in CR.VARIANTS}
    ref = runs["row-scalar"]
    assert ref[2:] == (8, 0) and ref[1][-1] < ref[1][0]
    for v, (x, h, it, conv) in runs.items():
        assert (it, conv) == (8, 0) and len(h) == 9 and np.all(np.isfinite(h)) and np.max(np.abs(h[:5] - ref[1][:5]) / ref[1][:5]) < 1e-10, v
    assert not same_bits(runs["stream"][1], runs["row-scalar"][1])    # fused partials against the streaming dot
    assert not same_bits(runs["adaptive"][1], runs["stream"][1])      # the hub rows' trees
    assert not same_bits(runs["wavefront"][1], runs["row-scalar"][1])
