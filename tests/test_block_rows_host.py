"""The block map's numpy restatement (tests/block_map.py) on hand-built cases, and where the names of the block-tile form live.
No GPU. The restatement is what tests/test_block_rows_gpu.py holds the library's maps against."""
import os
import re

import numpy as np
import pytest

import block_map as K
import tile_classes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slab_classes(O, e, n, world, rank):
    """Class map, first global grid row and grid rows of rank `rank` of a split into `world` slabs of whole grid rows."""
    rp, ci, va = O.build_csr(e, n * n)
    cut = [n * k // world for k in range(world + 1)]
    return T.classify(rp, ci, va, n, cut[rank] * n, (cut[rank + 1] - cut[rank]) * n)[0], cut[rank], cut[rank + 1] - cut[rank]


def by_hand(cls, gi_lo, gi_hi, R):
    """The definition, tile by tile: the set of (row block, col tile) that are fast."""
    fast = set()
    for b in range((gi_hi - gi_lo + R - 1) // R):
        rows = [gi_lo + b * R + r for r in range(R)]
        for t in range(cls.shape[1]):
            if all(li < gi_hi and cls[li, t] == 1 for li in rows):
                fast.add((b, t))
    return fast


def as_set(m):
    return {(int(b), int(t)) for b, t in np.argwhere(m == 1)}


@pytest.mark.parametrize("R", K.BLOCK_ROWS)
def test_generator_matrix_first_last_and_short_blocks_are_slow(O, R):
    """Whole grid, n = 130 (two column tiles, the last of two columns): the block that holds grid row 0 and the one that holds grid
    row n-1 are slow, so is the short last block (130 = 16 * 8 + 2 = 32 * 4 + 2), every other block is fast."""
    n = 130
    cls, gfirst, rows = slab_classes(O, O.stencil5_coo(n), n, 1, 0)
    m = K.block_map(cls, 0, rows, R)
    blocks = (n + R - 1) // R
    assert m.shape == (blocks, 2) and n % R == 2
    assert not m[0].any() and not m[blocks - 1].any() and m[1:blocks - 1].all()
    assert as_set(m) == by_hand(cls, 0, rows, R)


@pytest.mark.parametrize("R", K.BLOCK_ROWS)
def test_slabs_that_start_at_row_0_or_end_at_row_n_minus_1_and_their_interior_ranges(O, R):
    """Three slabs of whole grid rows of n = 640 (213 / 213 / 214 grid rows): the first slab's whole range starts with the grid's first grid row (a slow
    block), the last slab's ends with the grid's last (slow when the block is full, short otherwise); the interior ranges start one
    grid row later where a previous rank exists, so their blocks hold other rows than the whole range's."""
    n = 640
    e = O.stencil5_coo(n)
    for rank in range(3):
        cls, gfirst, rows = slab_classes(O, e, n, 3, rank)
        whole, interior = K.launch_ranges(rows, rank > 0, rank < 2)
        assert whole == (0, rows) and interior == (1 if rank > 0 else 0, rows - (1 if rank < 2 else 0))
        for lo, hi in (whole, interior):
            m = K.block_map(cls, lo, hi, R)
            assert as_set(m) == by_hand(cls, lo, hi, R)
            blocks = m.shape[0]
            short = (hi - lo) % R != 0
            first_slow = gfirst + lo == 0
            last_slow = short or gfirst + hi == n
            assert m[0].all() != first_slow and m[blocks - 1].all() != last_slow
            assert m[1:blocks - 1].all()


@pytest.mark.parametrize("R", K.BLOCK_ROWS)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_class_0_tile_makes_its_block_slow_whichever_row_of_the_block_holds_it(O, R, where):
    """A perturbed centre in the first, a middle and the last grid row of block 5 of the whole range (and only that tile's block)."""
    n = 300
    r = {"first": 0, "middle": R // 2, "last": R - 1}[where]
    gi, j = 5 * R + r, 200
    e = O.stencil5_coo(n)
    T.set_entry(e, gi * n + j, gi * n + j, 5.5)
    cls, gfirst, rows = slab_classes(O, e, n, 1, 0)
    assert cls[gi, 1] == 0 and cls[gi, 0] == 1 and cls[gi, 2] == 1
    m = K.block_map(cls, 0, rows, R)
    blocks = m.shape[0]
    slow = {(int(b), int(t)) for b, t in np.argwhere(m == 0)}
    assert slow == {(0, t) for t in range(3)} | {(blocks - 1, t) for t in range(3)} | {(5, 1)}
    # the same tile seen from a range that starts one grid row later sits in another row of (possibly another) block
    m1 = K.block_map(cls, 1, rows, R)
    assert m1[(gi - 1) // R, 1] == 0 and as_set(m1) == by_hand(cls, 1, rows, R)


def test_synthetic_maps():
    """No matrix: class maps written by hand."""
    cls = np.ones((9, 2), dtype=np.uint8)
    cls[6, 1] = 0
    assert K.block_map(cls, 0, 9, 4).tolist() == [[1, 1], [1, 0], [0, 0]]   # the last block holds one row
    assert K.block_map(cls, 1, 9, 4).tolist() == [[1, 1], [1, 0]]           # rows 1-4, 5-8
    assert K.block_map(cls, 0, 9, 8).tolist() == [[1, 0], [0, 0]]
    assert K.block_map(cls, 1, 9, 8).tolist() == [[1, 0]]
    assert K.block_map(cls, 0, 3, 4).tolist() == [[0, 0]]                   # a range shorter than one block
    assert K.block_map(cls, 2, 2, 4) is None and K.block_map(None, 0, 9, 4) is None and K.block_map(cls, 0, 9, 0) is None


def test_the_names_of_the_block_tile_form(B):
    """The map's export and the two options exist in the LAB build only; the product reads SPMV_AMD_ROWLDS_BLOCK_ROWS; both hold the
    block kernel under a symbol of its own, next to the one-row kernel's."""
    product = open(B.LIB_PATH, "rb").read()
    lab = open(B.LAB_LIB_PATH, "rb").read()
    for name in (b"spmv_amd_cg_slab_block_map", b"spmv_with_dot"):
        assert name not in product and name in lab, name
    assert "spmv_amd_cg_slab_block_map" in B.LAB_ONLY_SYMBOLS
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    assert re.search(r"^\s+spmv_amd_cg_slab_block_map;", open(os.path.join(csrc, "exports_lab.txt")).read(), flags=re.M)
    assert "spmv_amd_cg_slab_block_map" in open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    for binary in (product, lab):
        assert b"SPMV_AMD_ROWLDS_BLOCK_ROWS" in binary
        assert b"stencil5_rowlds_block_kernelILi4E" in binary and b"stencil5_rowlds_block_kernelILi8E" in binary
        assert b"stencil5_rowlds_kernelILi1E" in binary
