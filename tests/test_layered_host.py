"""tests/layered.py's matrices held against what they are meant to be, written out by hand (no GPU): the class-0 grid rows, the quintuple,
the uniform tile count, the slow / mixed row blocks of the block map for R = 4 and 8 and the cap 16 x slow <= blocks of
LoopShape::fused_direction, by tests/tile_classes.py and tests/block_map.py. A later edit of the builder cannot silently turn a case
into another one. tests/test_layered_gpu.py takes its expectations from EXPECTED.

A band holds WHOLE grid rows, so it turns every column tile of a row block it touches slow: a band that is not aligned to the row
blocks ("misaligned-640", and "r4-only-640" under R = 8) gives all-slow row blocks that also hold class-1 grid rows, never a mixed
row block. Those two cases therefore stay eligible for LoopShape::ap_recomputed; what they add is a slow block whose rows differ in
class. A mixed row block needs a perturbation narrower than the grid: mixed_coo below."""
import numpy as np
import pytest

import block_map as BM
import cg_restatement as CG
import layered as L
import tile_classes as T
from bitwise import same_bits

Q_BACKGROUND = (-1.25, 4.5, -1.25, -0.75, -0.75)  # W, C, E, N, S
Q_BAND = (-1.5, 6.0, -1.5, -1.0, -1.0)

# name -> quintuple, uniform tiles, {R: (slow row blocks, row blocks)}, {R: 16 x slow <= blocks}; by hand from the bands:
# the slow row blocks are those of grid rows 0 and n - 1 and those a band touches
EXPECTED = {
    "aniso-96": (Q_BACKGROUND, 94 * 1, {4: (2, 24), 8: (2, 12)}, {4: False, 8: False}),
    "aniso-129": (Q_BACKGROUND, 127 * 2, {4: (2, 33), 8: (2, 17)}, {4: True, 8: False}),
    "aniso-160": (Q_BACKGROUND, 158 * 2, {4: (2, 40), 8: (2, 20)}, {4: True, 8: False}),
    "aniso-257": (Q_BACKGROUND, 255 * 3, {4: (2, 65), 8: (2, 33)}, {4: True, 8: True}),
    "aniso-416": (Q_BACKGROUND, 414 * 4, {4: (2, 104), 8: (2, 52)}, {4: True, 8: True}),
    "layers-96": (Q_BACKGROUND, (94 - 8) * 1, {4: (4, 24), 8: (3, 12)}, {4: False, 8: False}),
    "layers-160": (Q_BACKGROUND, (158 - 24) * 2, {4: (8, 40), 8: (5, 20)}, {4: False, 8: False}),
    "layers-257": (Q_BACKGROUND, (255 - 8) * 3, {4: (4, 65), 8: (3, 33)}, {4: True, 8: False}),
    "layers-640": (Q_BACKGROUND, (638 - 24) * 5, {4: (8, 160), 8: (5, 80)}, {4: True, 8: True}),  # R = 8: 16 x 5 = 80, on the cap
    "misaligned-640": (Q_BACKGROUND, (638 - 8) * 5, {4: (5, 160), 8: (4, 80)}, {4: True, 8: True}),  # rows 82 .. 89: blocks 20-22 / 10, 11
    "r4-only-640": (Q_BACKGROUND, (638 - 4) * 5, {4: (3, 160), 8: (3, 80)}, {4: True, 8: True}),  # rows 84 .. 87: block 21 / half of 10
    "bad-pick-640": (Q_BAND, 6 * 5, {4: (160, 160), 8: (80, 80)}, {4: False, 8: False}),  # uniform: grid rows 317 .. 322
}
MIXED_SPOT = (200, 129)  # grid row, column of mixed_coo's one perturbed centre


def mixed_coo(O):
    """layers-640 with ONE centre changed (grid row 200, column tile 1): its row block has one slow block tile among fast ones, which
    switches LoopShape::ap_recomputed off. A copy: layered.case's arrays are shared."""
    n, e = L.case(O, "layers-640")[:2]
    e = e.copy()
    at = MIXED_SPOT[0] * n + MIXED_SPOT[1]
    T.set_entry(e, at, at, 4.75)
    return n, e


def row_block_states(cls, n, R):
    """(slow, mixed, all) row blocks of the whole-grid block map."""
    m = BM.block_map(cls, 0, n, R)
    fast, slow = (m == 1).all(axis=1), (m == 0).all(axis=1)
    return int(slow.sum()), int((~fast & ~slow).sum()), len(m), m


def test_the_table_names_every_case():
    assert set(EXPECTED) == set(L.CASES)


@pytest.mark.parametrize("name", list(L.CASES))
def test_a_case_is_what_the_table_says(O, name):
    n, e, rp, ci, va = L.case(O, name)
    want_q, want_uniform, want_blocks, want_cap = EXPECTED[name]
    bands = L.band_rows(name)
    assert same_bits(T.quintuple(rp, va, n, 0, n * n), want_q)
    sampled = 1 + (n - 2) // 2
    assert (sampled in bands) == (name == "bad-pick-640")
    cls, uniform, total = T.classify(rp, ci, va, n, 0, n * n)
    ct = T.col_tiles(n)
    assert (uniform, total) == (want_uniform, (n - 2) * ct)
    assert ((cls == 1).all(axis=1) | (cls == 0).all(axis=1)).all()  # no grid row has tiles of both classes
    class0 = np.flatnonzero((cls == 0).all(axis=1)).tolist()
    if name == "bad-pick-640":
        assert class0 == [gi for gi in range(n) if not 317 <= gi <= 322]
    else:
        assert class0 == sorted([0, n - 1] + bands)
    for R in BM.BLOCK_ROWS:
        slow, mixed, blocks, m = row_block_states(cls, n, R)
        assert (slow, blocks) == want_blocks[R] and mixed == 0, (R, slow, mixed, blocks)
        assert blocks == -(-n // R) and m.shape[1] == ct
        assert (16 * int((m == 0).sum()) <= m.size) == (16 * slow <= blocks) == want_cap[R], R
        by_hand = sorted({0, (n - 1) // R} | {gi // R for gi in bands}) if name != "bad-pick-640" else list(range(blocks))
        assert np.flatnonzero((m == 0).all(axis=1)).tolist() == by_hand, R


def test_the_values_of_a_layered_matrix(O):
    """layers-96 entry by entry against the rule, stated as a loop over the entries: centre / horizontal / vertical by position, the
    band's values where BOTH ends lie inside it. And the matrix is bitwise symmetric and strictly diagonally dominant."""
    n, e = L.case(O, "layers-96")[:2]
    lo, hi = L.CASES["layers-96"][1][0]
    entries = {}
    for row, col, value in zip(e["row"].tolist(), e["col"].tolist(), e["value"].tolist()):
        gi, gj = row // n, col // n
        c, h, v = L.BAND if lo <= gi < hi and lo <= gj < hi else L.BACKGROUND
        assert value == (c if row == col else h if gi == gj else v), (row, col)
        entries[row, col] = value
    assert len(entries) == len(e)
    off = np.zeros(n * n)
    for (row, col), value in entries.items():
        assert entries[col, row] == value
        if row != col:
            off[row] += abs(value)
    assert all(entries[k, k] > off[k] for k in range(n * n))
    assert entries[39 * n + 5, 40 * n + 5] == -0.75 and entries[40 * n + 5, 41 * n + 5] == -1.0 and entries[47 * n + 5, 48 * n + 5] == -0.75
    assert entries[40 * n + 5, 40 * n + 6] == -1.5 and entries[39 * n + 5, 39 * n + 6] == -1.25


def test_every_case_is_symmetric_and_diagonally_dominant(O):
    for name in L.CASES:
        n, e = L.case(O, name)[:2]
        row, col, value = e["row"].astype(np.int64), e["col"].astype(np.int64), e["value"]
        order, mirror = np.lexsort((col, row)), np.lexsort((row, col))
        assert np.array_equal(row[order], col[mirror]) and np.array_equal(col[order], row[mirror])
        assert same_bits(value[order], value[mirror]), name
        off = np.bincount(row[row != col], weights=np.abs(value[row != col]), minlength=n * n)
        assert (value[row == col][np.argsort(row[row == col])] > off).all(), name


def test_the_mixed_matrix_has_one_mixed_row_block(O):
    n, e = mixed_coo(O)
    rp, ci, va = O.build_csr(e, n * n)
    cls = T.classify(rp, ci, va, n, 0, n * n)[0]
    assert np.argwhere((cls == 0) & (cls.sum(axis=1, keepdims=True) > 0)).tolist() == [[MIXED_SPOT[0], MIXED_SPOT[1] // T.TILE]]
    for R in BM.BLOCK_ROWS:
        slow, mixed, blocks, m = row_block_states(cls, n, R)
        assert (slow, mixed) == (EXPECTED["layers-640"][2][R][0], 1) and m[MIXED_SPOT[0] // R].sum() == T.col_tiles(n) - 1


@pytest.mark.parametrize("name", ["layers-96", "layers-160", "layers-257", "layers-640"])
def test_the_restated_solve_converges(O, name):
    """Random b, x0 = 0, tolerance 1e-8: the condition number is that of a strictly diagonally dominant stencil whatever the grid, so
    the iteration count does not grow with n (about 40; more than the direction ring's 16 slots, which the GPU solves rely on)."""
    n, _, rp, ci, va = L.case(O, name)
    b = np.random.default_rng(n).standard_normal(n * n)
    x, history, iterations, converged = CG.solve(CG.whole_grid(O, rp, ci, va, n, "row-lds"), b, np.zeros(n * n), 300, 1e-8)
    assert converged == 1 and 32 < iterations < 56, iterations
    residual = b - O.spmv_stencil5(rp, ci, va, x, n)
    assert np.linalg.norm(residual) < 2e-8 * np.linalg.norm(b)
