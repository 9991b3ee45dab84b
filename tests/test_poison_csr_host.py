"""The general-CSR section of tests/poison.py on the CPU alone: the level made for the AMG restriction holds every seam it is named
for; the reference's non-finite coarse rows are exactly the planted set of every case, most coarse rows stay finite and every target
has a finite neighbour in its wave, so tests/test_poison_csr_gpu.py cannot pass by comparing NaN with NaN; the prolongation's levels
and the two matrices "as a file gives them" are what they claim; and the cases discriminate, shown with deliberately wrong numpy
models of the two transfers and not with wrong kernels on a GPU. Each model agrees bit for bit with the reference on the finite data
the stage tests use (tests/test_amg_stages_gpu.py, level_for(513)), so the suite could not see it before, and differs from the
reference on the new table:

    model                                                           caught by
    leak    an absent lane reads the next member row, its t is      r_inf, z_inf, coef_inf (a NaN beside the target: 0.0 * inf),
            multiplied by 0.0 and added                             negzero_sum, negzero_chain (-0.0 + +0.0 is +0.0)
    zero    acc starts at +0.0                                      negzero_sum, negzero_chain (+0.0 + -0.0 is +0.0)
    first   the row chain starts from its first product             negzero_chain (the bare product -0.0 makes t = +0.0)
    pair    a 16-byte pair takes its first row's aggregate          the inf cases of prolong_level(2, 3, 129, 4225)

No tolerance anywhere: bit patterns and NaN classes."""
import functools

import numpy as np
import pytest

import amg_restatement as AMG
import poison as P
from bitwise import same_bits, same_bits_nan_as_class

GROUPS = 8  # aggregates per wave, lanes per aggregate


# ---------------------------------------------------------------- the level
def test_the_level_holds_every_seam():
    L = P.aggregate_level()
    sizes = np.diff(L.agg_ptr).tolist()
    assert L.count == 29 and sizes == [s for wave in P.AGG_WAVES for s in wave] and len(L.rp) - 1 == sum(sizes) + 5
    assert [len(w) for w in P.AGG_WAVES] == [8, 8, 8, 5]  # three dead groups in the last wave
    assert len(L.free_rows) == 5 and (L.agg[L.free_rows] == -1).all() and not np.isin(L.free_rows, L.members).any()
    assert sorted(L.members.tolist()) == sorted(np.flatnonzero(L.agg >= 0).tolist())
    for I in range(L.count):
        m = L.members[L.agg_ptr[I]:L.agg_ptr[I + 1]]
        assert (np.diff(m) > 0).all() and (L.agg[m] == I).all()
    # dealt at random: the members of an aggregate are no run of neighbouring rows
    assert np.diff(P.target_members((0, 0))).max() > 1
    lengths = np.diff(L.rp)
    assert set(lengths.tolist()) == {0, 1, 5, 70} and {0, 1, 5, 70} <= set(lengths[L.members].tolist())
    assert (L.va >= 0.25).all() and (L.va < 3.0).all() and np.isfinite(L.z).all() and np.isfinite(L.r).all() and (L.z != 0.0).all()
    rows = P.row_of_entry(L.rp)
    assert all((np.diff(L.ci[L.rp[i]:L.rp[i + 1]]) > 0).all() for i in range(len(L.rp) - 1))
    # the reserved band: behind the pool, one column per non-empty member row of a target, each referred to by that row alone
    held = np.flatnonzero(L.reserved >= 0)
    want = np.concatenate([m[lengths[m] > 0] for m in (P.target_members(t) for t in P.AGG_TARGETS)])
    assert sorted(held.tolist()) == sorted(want.tolist())
    assert sorted(L.reserved[held].tolist()) == list(range(P.AGG_POOL, L.cols))
    for row in held:
        at = np.flatnonzero(L.ci == L.reserved[row])
        assert len(at) == 1 and rows[at[0]] == row and at[0] == L.rp[row + 1] - 1
    # the targets and their slots
    assert [len(P.target_members(t)) for t in P.AGG_TARGETS] == [100, 1, 100, 8, 8, 9]
    assert P.target_slots((0, 0)) == ["all", 0, 7, 8, 99] and P.target_slots((0, 1)) == [0] and P.target_slots((1, 3)) == ["all", 0, 7, 8]
    assert P.target_slots((2, 0)) == P.target_slots((3, 4)) == ["all", 0, 7]
    assert P.coarse_of((1, 7)) + 1 == P.coarse_of((2, 0)) and P.coarse_of((3, 4)) == L.count - 1  # a wave seam; the last live group
    for t in P.AGG_TARGETS:
        m = P.target_members(t)
        assert all(lengths[m[s]] > 0 for s in P.target_slots(t) if s != "all"), t
    assert len(P.AGG_TABLE) == len(set(P.AGG_TABLE)) == 85


def test_the_clean_level_is_finite():
    assert np.isfinite(P.aggregate_reference()).all()


# ---------------------------------------------------------------- adjacency and coverage
@pytest.mark.parametrize("planter", P.AGG_PLANTERS)
def test_the_non_finite_coarse_rows_are_the_planted_set(planter):
    """For every target and slot: the reference's non-finite coarse rows are exactly the planted set, which is the target alone (the
    signed-zero planters: nobody); r_inf gives +inf and z_inf -inf, never a NaN, so inf - inf does not occur inside an aggregate; at
    least three quarters of the coarse rows are finite; the target has a finite neighbour in its own wave; and every coarse row whose
    inputs are the clean level's has the clean bits."""
    L = P.aggregate_level()
    clean = P.aggregate_reference()
    cases = P.aggregate_cases(planter)
    assert len(cases) >= len(P.AGG_TARGETS)
    for _, target, slot in cases:
        c, ref = P.aggregate_case(planter, target, slot), P.aggregate_reference(planter, target, slot)
        I = P.coarse_of(target)
        bad = np.flatnonzero(~np.isfinite(ref))
        assert np.array_equal(bad, c.planted), (planter, target, slot, bad, c.planted)
        # the planted set once more, written out: the aggregates of the rows that were planted at
        inf = planter.endswith("_inf")
        assert c.planted.tolist() == ([I] if inf else []) and (not inf or set(L.agg[c.rows_at].tolist()) == {I})
        if planter == "r_inf":
            assert np.isposinf(c.r[c.rows_at]).all() and int(np.isinf(c.r).sum()) == len(c.rows_at) and ref[I] == np.inf
        elif planter == "z_inf":
            at = np.flatnonzero(np.isinf(c.z))
            assert np.array_equal(np.sort(L.reserved[c.rows_at]), at) and np.isposinf(c.z[at]).all() and ref[I] == -np.inf
        elif planter == "coef_inf":
            at = np.flatnonzero(np.isinf(c.va))
            assert np.array_equal(np.unique(P.row_of_entry(c.rp)[at]), np.sort(c.rows_at)) and len(at) == len(c.rows_at)
        else:
            m = P.target_members(target)
            assert same_bits(c.r[m], np.full(len(m), -0.0)) and same_bits([ref[I]], [-0.0]), (planter, target, slot, ref[I])
            kept = np.flatnonzero(np.diff(c.rp)[m] > 0)
            assert kept.tolist() == ([] if planter == "negzero_sum" else [slot])
            if planter == "negzero_chain":
                cols = c.ci[c.rp[m[slot]]:c.rp[m[slot] + 1]]
                assert len(cols) in (1, 5, 70) and same_bits(c.z[cols], np.full(len(cols), -0.0))
        if planter in ("r_inf", "z_inf"):
            assert not np.isnan(ref).any(), (planter, target, slot)
        assert 4 * int(np.isfinite(ref).sum()) >= 3 * L.count
        wave = np.arange(GROUPS * target[0], min(GROUPS * (target[0] + 1), L.count))
        assert np.isfinite(ref[wave[wave != I]]).any(), (planter, target, slot)
        outside = np.setdiff1d(np.arange(L.count), c.touched)
        # (negzero_chain's -0.0 sits in pool columns other rows hold too: a 70-entry row touches most of the level)
        assert I in c.touched and (len(c.touched) == 1 or planter == "negzero_chain") and len(outside) > 0
        assert same_bits(ref[outside], clean[outside])


# ---------------------------------------------------------------- wrong models of the restriction
def row_terms(O, rp, ci, va, z, r, first_product=False):
    """t = fma(-1.0, s, r) per row. s is the sequential chain from +0.0 (the oracle's) or, first_product, a WRONG chain that starts
    from the bare product of the row's first entry."""
    if not first_product:
        return O.axpy(-1.0, O.spmv_csr(rp, ci, va, z), r)
    rows = len(rp) - 1
    length = np.diff(rp)
    s = np.zeros(rows)
    for k in range(int(length.max())):
        live = np.flatnonzero(length > k)
        at = rp[live] + k
        s[live] = va[at] * z[ci[at]] if k == 0 else O.fma(va[at], z[ci[at]], s[live])
    return O.axpy(-1.0, s, r)


def restrict_model(t, agg_ptr, members, leak=False, zero=False):
    """The kernel's walk: eight aggregates per wave, the round count the wave's maximum, eight members per round, the sum in member
    order from the first member's t. leak (WRONG): an absent lane takes the member list's next row -- the next aggregate's -- and its
    t is multiplied by 0.0 and added. zero (WRONG): acc starts at +0.0."""
    count = len(agg_ptr) - 1
    out = np.zeros(count)
    with np.errstate(invalid="ignore"):
        for wave in range(0, count, GROUPS):
            groups = range(wave, min(wave + GROUPS, count))
            rounds = max((int(agg_ptr[I + 1] - agg_ptr[I]) + GROUPS - 1) // GROUPS for I in groups)
            for I in groups:
                m0, m1 = int(agg_ptr[I]), int(agg_ptr[I + 1])
                acc = np.float64(0.0)
                for rnd in range(rounds):
                    begin = m0 + GROUPS * rnd
                    have = m1 - begin
                    for q in range(GROUPS):
                        if q < have:
                            tq = t[members[begin + q]]
                            acc = tq if (rnd == 0 and q == 0 and not zero) else acc + tq
                        elif leak:
                            tq = t[members[begin + q]] if begin + q < len(members) else np.float64(0.0)
                            acc = acc + np.float64(0.0) * tq
                out[I] = acc
    return out


RESTRICT_MODELS = {"leak": dict(leak=True), "zero": dict(zero=True), "first": dict(first_product=True)}
CATCHES = {"leak": set(P.AGG_PLANTERS), "zero": {"negzero_sum", "negzero_chain"}, "first": {"negzero_chain"}}  # the docstring's table


def model_of(O, name, rp, ci, va, z, r, agg_ptr, members):
    flags = RESTRICT_MODELS.get(name, {})
    t = row_terms(O, rp, ci, va, z, r, flags.get("first_product", False))
    return restrict_model(t, agg_ptr, members, flags.get("leak", False), flags.get("zero", False))


@functools.lru_cache(maxsize=1)
def old_level():
    from test_amg_stages_gpu import level_for
    return level_for(513)


def test_the_right_model_is_the_reference(O):
    """The walk itself, with no flag set, is amg_restatement.restrict bit for bit: on the old data and on every case of the table."""
    M, g, z, r, _ = old_level()
    want = AMG.restrict(O.axpy(-1.0, O.spmv_csr(M.rp, M.ci, M.va, z), r), g)
    assert np.isfinite(want).all() and same_bits(model_of(O, None, M.rp, M.ci, M.va, z, r, g.agg_ptr, g.members), want)
    L = P.aggregate_level()
    for case in P.AGG_TABLE:
        c = P.aggregate_case(*case)
        assert same_bits_nan_as_class(model_of(O, None, c.rp, c.ci, c.va, c.z, c.r, L.agg_ptr, L.members), P.aggregate_reference(*case)), case


@pytest.mark.parametrize("model", sorted(RESTRICT_MODELS))
def test_a_wrong_restriction_is_invisible_to_the_old_data_and_caught_by_the_table(O, model):
    M, g, z, r, _ = old_level()
    want = AMG.restrict(O.axpy(-1.0, O.spmv_csr(M.rp, M.ci, M.va, z), r), g)
    assert same_bits(model_of(O, model, M.rp, M.ci, M.va, z, r, g.agg_ptr, g.members), want), "the old data would have caught it"
    L = P.aggregate_level()
    caught = {}
    for case in P.AGG_TABLE:
        c, ref = P.aggregate_case(*case), P.aggregate_reference(*case)
        got = model_of(O, model, c.rp, c.ci, c.va, c.z, c.r, L.agg_ptr, L.members)
        try:
            same_bits_nan_as_class(got, ref)
        except AssertionError:
            caught.setdefault(case[0], []).append(case[1:])
    print(model, {k: len(v) for k, v in caught.items()})
    assert set(caught) == CATCHES[model], (model, sorted(caught))
    if model == "leak":
        # this model reads forward in the member list, so a poison shows in the aggregates in front of its own: every target of the
        # inf planters is caught at some slot but aggregate 0, which has nobody in front of it (it is there for the other direction:
        # the seven singles beside it run twelve rounds at have <= 0)
        for planter in ("r_inf", "z_inf", "coef_inf"):
            assert {t for t, _ in caught[planter]} == {t for t in P.AGG_TARGETS if P.coarse_of(t) > 0}, (planter, caught[planter])
    else:  # the signed zeros: every case of the catching planters
        for planter in CATCHES[model]:
            assert len(caught[planter]) == len(P.aggregate_cases(planter)), (model, planter)


# ---------------------------------------------------------------- the prolongation
def prolong_model(O, agg, ec, z, pair_takes_first=False):
    """z = fma(2.0, e_c[agg], z). pair_takes_first (WRONG): rows 2 i and 2 i + 1 both take agg[2 i]; the odd last row its own."""
    use = np.array(agg, dtype=np.int64)
    if pair_takes_first:
        pairs = len(agg) // 2
        use[1:2 * pairs:2] = use[0:2 * pairs:2]
    return O.axpy(2.0, np.ascontiguousarray(ec[use]), z)


@pytest.mark.parametrize("rows", P.PROLONG_ROWS)
def test_the_prolongation_levels_and_their_wrong_model(O, rows):
    L = P.prolong_level(rows)
    assert len(L.agg) == rows and set(L.agg.tolist()) == set(range(L.coarse_rows))  # no aggregate is empty
    if rows > 1:
        assert L.agg[0] != L.agg[1]  # the two rows of a 16-byte pair in different aggregates
    if rows >= 129:
        assert 2 * int(np.sum(L.agg[0:rows - 1:2] != L.agg[1:rows:2])) > rows // 2  # most pairs
    cases = P.prolong_cases(rows)
    assert [I for _, _, _, I in cases] == sorted({0, L.coarse_rows // 2, L.coarse_rows - 1}) + [None]
    caught = 0
    for label, ec, z, I in cases:
        want = prolong_model(O, L.agg, ec, z)
        if I is None:
            assert same_bits(want, np.full(rows, -0.0))
        else:
            assert np.array_equal(np.flatnonzero(~np.isfinite(want)), np.flatnonzero(L.agg == I)) and (want[L.agg == I] == np.inf).all()
            keep = L.agg != I
            assert same_bits(want[keep], prolong_model(O, L.agg, L.ec, L.z)[keep])
        wrong = prolong_model(O, L.agg, ec, z, pair_takes_first=True)
        caught += not same_bits(wrong, want)
    assert caught >= (1 if rows > 1 else 0), rows  # rows = 1: no pair, the model is right there
    if rows > 1:
        assert caught == len(cases) - 1 or rows <= 3  # -0.0 everywhere cannot show an index; at 129 and 4 225 every inf case does
    # invisible where the pairs share an aggregate: the model is the reference bit for bit, inf or not
    shared = np.repeat(np.arange((rows + 1) // 2), 2)[:rows].astype(np.int32) % L.coarse_rows
    for label, ec, z, I in cases:
        assert same_bits(prolong_model(O, shared, ec, z, pair_takes_first=True), prolong_model(O, shared, ec, z)), (rows, label)


# ---------------------------------------------------------------- the matrices as a file gives them
def stored_pairs(M):
    """Indices k with entry k and k + 1 in the same row and column."""
    rows = AMG.row_index(M)
    return np.flatnonzero((rows[1:] == rows[:-1]) & (M.ci[1:] == M.ci[:-1]))


def summed(M):
    A = AMG.scipy_of(M).copy()
    A.sum_duplicates()
    return A


@pytest.mark.parametrize("name", ["split33", "oneway33"])
def test_the_matrices_hold_what_they_claim(name):
    M = AMG.as_a_file_gives_it(name)
    n = AMG.rows_of(M)
    rows = AMG.row_index(M)
    assert n == 33 * 33 and all((np.diff(M.ci[M.rp[i]:M.rp[i + 1]]) >= 0).all() for i in range(n))  # sorted, equal columns adjacent
    pairs = stored_pairs(M)
    assert len(pairs) > 1000, "duplicates exist"
    zeros = np.flatnonzero(M.va == 0.0)
    assert len(zeros) > 500 and all(k in pairs or k - 1 in pairs for k in zeros), "stored zeros exist, each beside a live twin"
    assert (np.isin(zeros, pairs).sum() > 100) and (np.isin(zeros - 1, pairs).sum() > 100)  # in front of the twin and behind it
    split = pairs[(M.va[pairs] != 0.0) & (M.va[pairs + 1] != 0.0)]
    quarter = split[M.va[split] * 3.0 == M.va[split + 1]]
    assert len(quarter) > 500, "entries split into v / 4 and 3 v / 4"
    assert (M.ci[pairs] == rows[pairs]).sum() > 100  # on the diagonal too
    assert same_bits(AMG.diagonal(M), np.full(n, 4.0))  # the diagonal is the sum of the row's parts in column i
    A, poisson = summed(M), AMG.scipy_of(AMG.poisson2d(33))
    if name == "split33":
        assert abs(A - poisson).max() == 0.0 and abs(A - A.T).max() == 0.0  # sums exactly to Poisson: symmetric positive definite
        assert len(split) == len(quarter)
    else:
        cancel = split[(M.va[split] == -1.5 * M.va[split + 1])]
        assert len(cancel) > 100 and set(M.va[cancel].tolist()) <= {12.0, -3.0}, "partly cancelling pairs (3 v, -2 v)"
        pattern = (A != 0).astype(np.int8)
        one_way = (pattern - pattern.T)
        assert (one_way != 0).nnz > 100 and abs(A - A.T).max() == 1.0, "the pattern is not symmetric"
        dropped = poisson.nnz - (A != 0).sum()
        assert 0.04 * (poisson.nnz - n) / 2 < dropped < 0.10 * (poisson.nnz - n) / 2  # about 7 % of the edges, one side each
        kept = (A != 0).multiply(poisson != 0)
        assert abs(A - poisson.multiply(kept)).max() == 0.0  # every entry that is left sums to Poisson's


@pytest.mark.parametrize("name", ["split33", "oneway33"])
def test_lambda_max_is_the_raw_csr_row_sum(name):
    """Every level of the hierarchy: the restatement's lambda_max against max_i sum_k |v_k| sqrt(|dinv_i| |dinv_col(k)|) written out
    here over the raw CSR arrays, each stored part a term of its own, in CSR order from 0.0."""
    levels = AMG.hierarchy(AMG.as_a_file_gives_it(name), 1)
    assert [L.rows for L in levels] == {"split33": [1089, 195, 28], "oneway33": [1089, 198, 30]}[name]
    for l, L in enumerate(levels):
        M = L.M
        d = np.zeros(L.rows)
        for i in range(L.rows):
            for k in range(M.rp[i], M.rp[i + 1]):
                if M.ci[k] == i:
                    d[i] = d[i] + M.va[k]
        assert same_bits(1.0 / d, L.dinv), (name, l)
        best = 0.0
        for i in range(L.rows):
            s = 0.0
            for k in range(M.rp[i], M.rp[i + 1]):
                s = s + abs(M.va[k]) * np.sqrt(abs(L.dinv[i]) * abs(L.dinv[M.ci[k]]))
            best = max(best, s)
        assert same_bits([best], [L.lambda_max]), (name, l, best, L.lambda_max)
    if name == "split33":  # the split parts are terms of their own: |v/4| + |3v/4| = |v| exactly, a 0.0 adds nothing
        assert same_bits([levels[0].lambda_max], [AMG.hierarchy(AMG.poisson2d(33), 1)[0].lambda_max])


def test_shuffled_entries_come_back_sorted_with_their_duplicates():
    """csr_of_entries (what build_csr_struct makes of a shuffled file): the same rows and columns as the sorted form, the values of a
    duplicate pair in either order, nothing merged."""
    for name, seed in (("split33", 41), ("oneway33", 42)):
        M = AMG.as_a_file_gives_it(name)
        e = P.shuffled_entries(M.rp, M.ci, M.va, seed)
        assert not np.array_equal(e["row"], P.entries_of(M.rp, M.ci, M.va)["row"])
        rp, ci, va = P.csr_of_entries(e, AMG.rows_of(M))
        assert np.array_equal(rp, M.rp) and np.array_equal(ci, M.ci) and not same_bits(va, M.va)
        pairs = stored_pairs(M)
        swapped = (va[pairs] == M.va[pairs + 1]) & (va[pairs + 1] == M.va[pairs])
        stayed = (va[pairs] == M.va[pairs]) & (va[pairs + 1] == M.va[pairs + 1])
        assert (swapped | stayed).all() and (swapped & ~stayed).any() and stayed.any()
        lone = np.ones(len(ci), dtype=bool)
        lone[pairs], lone[pairs + 1] = False, False
        assert same_bits(va[lone], M.va[lone])
        assert same_bits(AMG.diagonal(AMG.Csr(rp, ci, va)), AMG.diagonal(M))
