"""Anisotropic and layered 5-point stencils for the CG slab's uniform-tile loop (tests/test_layered_host.py, tests/test_layered_gpu.py).
Test infrastructure only.

The generator's matrix has four equal off-diagonals, so a fast path that hands one member of the quintuple (W, C, E, N, S) where
another belongs computes the same bits. Here the horizontal and the vertical coupling differ (W = E != N = S), and BANDS of whole grid
rows carry coefficients of their own: a band that fills whole row blocks makes them all-slow in the INTERIOR of the grid, which keeps
LoopShape::ap_recomputed eligible (csrc/skew_geometry.hpp skew_eligible) while its r update reads a stored A p' next to recomputed
ones. Every matrix is bitwise symmetric and strictly diagonally dominant (4.5 > 2 * 1.25 + 2 * 0.75, 6.0 > 2 * 1.5 + 2 * 1.0; a row
at a band's border 6.0 > 2 * 1.5 + 1.0 + 0.75), hence SPD."""
import numpy as np

BACKGROUND = (4.5, -1.25, -0.75)  # centre, horizontal, vertical
BAND = (6.0, -1.5, -1.0)

# name -> (n, bands [lo, hi) of grid rows)
CASES = {
    "aniso-96": (96, ()),
    "aniso-129": (129, ()),
    "aniso-160": (160, ()),
    "aniso-257": (257, ()),
    "aniso-416": (416, ()),
    "layers-96": (96, ((40, 48),)),
    "layers-160": (160, ((40, 48), (96, 112))),
    "layers-257": (257, ((64, 72),)),
    "layers-640": (640, ((80, 88), (304, 320))),
    "misaligned-640": (640, ((82, 90),)),
    "r4-only-640": (640, ((84, 88),)),
    "bad-pick-640": (640, ((316, 324),)),
}
_cache = {}


def layered_coo(O, n, c, h, v, bands=()):
    """O.stencil5_coo(n)'s pattern with centre c, horizontal edges h and vertical edges v; for each band (lo, hi, bc, bh, bv) of whole
    grid rows [lo, hi): centres of those rows bc, horizontal edges inside them bh, vertical edges with BOTH ends inside bv. A vertical
    edge across a band's border keeps v, so the rows outside a band are untouched."""
    e = O.stencil5_coo(n)
    row, col = e["row"].astype(np.int64), e["col"].astype(np.int64)
    centre, horizontal, vertical = row == col, np.abs(row - col) == 1, np.abs(row - col) == n
    assert n >= 3 and (centre | horizontal | vertical).all()
    value = np.where(centre, c, np.where(horizontal, h, v)).astype(np.float64)
    gi, gj = row // n, col // n  # the grid rows of both ends
    for lo, hi, bc, bh, bv in bands:
        assert 0 <= lo < hi <= n
        inside = (gi >= lo) & (gi < hi) & (gj >= lo) & (gj < hi)
        value[inside] = np.where(centre[inside], bc, np.where(horizontal[inside], bh, bv))
    e["value"] = value
    return e


def band_rows(name):
    """The grid rows inside the bands of a case, by hand from the table."""
    return sorted(gi for lo, hi in CASES[name][1] for gi in range(lo, hi))


def case(O, name):
    """(n, COO entries, rp, ci, va) of a case of the table: built once, shared, never written."""
    if name not in _cache:
        n, bands = CASES[name]
        e = layered_coo(O, n, *BACKGROUND, [(lo, hi) + BAND for lo, hi in bands])
        _cache[name] = (n, e) + tuple(O.build_csr(e, n * n))
    return _cache[name]
