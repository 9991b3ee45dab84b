"""numpy restatement of the CG slab's block maps (csrc/spmv_kernels.hip block_map_kernel, csrc/cg_slab_create.hip build_block_maps;
kernels.hpp Stencil5Plan). Test infrastructure only.

The in-loop SpMV evaluates BLOCK TILES: 128 columns x R consecutive local grid rows, counted from the first grid row of the launch
range. A block is FAST (1) when it holds R rows of the range and every one of its R row-lds tiles is class 1 in the slab's class map
(tests/tile_classes.py); every other block -- one with a class-0 tile, one that holds the grid's first or last grid row (never
class 1), the short last block of a range -- is evaluated row by row (0). A slab has two ranges: the whole slab, and the rows that
need no halo (all but the first local grid row where a previous rank exists, all but the last where a next rank exists)."""
import numpy as np

BLOCK_ROWS = (4, 8)


def launch_ranges(rows, has_prev, has_next):
    """[gi_lo, gi_hi) in local grid rows of the two launch ranges of a slab of `rows` grid rows: (whole, interior)."""
    return (0, rows), (1 if has_prev else 0, rows - (1 if has_next else 0))


def block_map(cls, gi_lo, gi_hi, R):
    """uint8 [row blocks, col tiles] of the range [gi_lo, gi_hi) of a slab whose class map is `cls` ([local grid rows, col tiles]),
    or None where the library keeps no map (no class map, R = 0, an empty range)."""
    if cls is None or R <= 0 or gi_hi <= gi_lo:
        return None
    blocks = (gi_hi - gi_lo + R - 1) // R
    out = np.zeros((blocks, cls.shape[1]), dtype=np.uint8)
    for b in range(blocks):
        lo = gi_lo + b * R
        if lo + R <= gi_hi:
            out[b] = (cls[lo:lo + R] == 1).all(axis=0)
    return out


def row_counts(rows, has_prev, has_next):
    """The row counts of the two ranges (what the remainders modulo R are taken of)."""
    return [hi - lo for lo, hi in launch_ranges(rows, has_prev, has_next)]
