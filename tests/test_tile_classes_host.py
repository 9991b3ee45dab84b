"""The tile classifier's numpy restatement (tests/tile_classes.py) on hand-built cases, and where the two LAB-only names of the
uniform-tile form live. No GPU. The restatement is what tests/test_uniform_tiles_gpu.py holds the library's map against."""
import numpy as np

import tile_classes as T


def csr_of(O, e, n):
    return O.build_csr(e, n * n)


def whole(n):
    return 0, n * n


def test_generator_matrix_is_uniform_everywhere_with_both_column_exemptions(O):
    """Column 0 has no W and column n-1 has no E, and the last tile ends at column n (n = 300: 44 of its 128 columns exist):
    none of that may cost a tile its class. Grid rows 0 and n-1 are class 0 and are not counted."""
    for n in (130, 300, 640):
        rp, ci, va = O.stencil5_csr(n)
        cls, uniform, total = T.classify(rp, ci, va, n, *whole(n))
        ct = T.col_tiles(n)
        assert cls.shape == (n, ct) and total == (n - 2) * ct and uniform == total
        assert not cls[0].any() and not cls[n - 1].any() and cls[1:n - 1].all()
        assert np.array_equal(T.quintuple(rp, va, n, *whole(n)), [-1.0, 5.0, -1.0, -1.0, -1.0])


def test_slabs_count_only_their_plane_evaluated_grid_rows(O):
    n = 640
    rp, ci, va = O.stencil5_csr(n)
    ct = T.col_tiles(n)
    for world in (1, 2, 4):
        for rank in range(world):
            off, nl = O.partition_rows(n * n, world, rank)
            cls, uniform, total = T.classify(rp, ci, va, n, off, nl)
            rows = nl // n - (1 if rank == 0 else 0) - (1 if rank == world - 1 else 0)
            assert cls.shape == (nl // n, ct) and uniform == total == rows * ct
    # a slab that is only the grid's first grid row has nothing evaluated from the planes: no map
    assert T.classify(rp, ci, va, n, 0, n) == (None, 0, 0)


def flipped(O, e, n, off=0, nl=None):
    rp, ci, va = csr_of(O, e, n)
    cls, uniform, total = T.classify(rp, ci, va, n, off, n * n if nl is None else nl)
    gfirst = off // n
    zeros = {(gfirst + int(r), int(t)) for r, t in np.argwhere(cls == 0)} - {(0, t) for t in range(T.col_tiles(n))} - {(n - 1, t) for t in range(T.col_tiles(n))}
    assert uniform == total - len(zeros)
    return zeros


def test_the_coefficients_a_boundary_column_does_use_count(O):
    """A CSR cannot hold a W entry in column 0 or an E entry in column n-1, so the exemption is tested from the other side: the N
    entry of column 0 and the W entry of column n-1 ARE multiplied, and a change there costs the tile its class."""
    n = 300
    e = O.stencil5_coo(n)
    T.set_edge(e, 40 * n, 39 * n, -1.5)                       # N of (40, 0) = S of (39, 0)
    T.set_edge(e, 80 * n + n - 1, 80 * n + n - 2, -1.5)       # W of (80, n-1) = E of (80, n-2)
    assert flipped(O, e, n) == {(40, 0), (39, 0), (80, 2)}


def test_signed_zero_and_one_ulp_are_not_the_quintuple(O):
    """Bit patterns, not ==: with every horizontal edge +0.0, one edge at -0.0 (equal under ==) flips its tile; so does a value 1 ulp
    off. Both changes are kept symmetric."""
    n = 300
    e = O.stencil5_coo(n)
    horizontal = np.abs(e["row"].astype(np.int64) - e["col"].astype(np.int64)) == 1
    e["value"][horizontal] = 0.0
    rp, ci, va = csr_of(O, e, n)
    assert T.classify(rp, ci, va, n, *whole(n))[1] == (n - 2) * T.col_tiles(n)
    T.set_edge(e, 50 * n + 10, 50 * n + 11, -0.0)
    assert flipped(O, e, n) == {(50, 0)}
    e = O.stencil5_coo(n)
    T.set_edge(e, 60 * n + 200, 61 * n + 200, np.nextafter(-1.0, 0.0))
    T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
    assert flipped(O, e, n) == {(60, 1), (61, 1), (70, 1)}


def test_first_local_grid_row_of_a_slab_takes_its_own_north_entries(O):
    """A vertical edge across the P = 2 cut: the lower slab's first local grid row holds the changed N entry in its own CSR rows, the
    upper slab's last grid row the changed S entry; each slab's map shows one class-0 tile."""
    n = 640
    e = O.stencil5_coo(n)
    T.set_edge(e, 319 * n + 500, 320 * n + 500, -1.25)
    half = n * n // 2
    assert flipped(O, e, n, 0, half) == {(319, 3)}
    assert flipped(O, e, n, half, half) == {(320, 3)}


def test_mixed_matrix_has_both_classes_in_every_slab_it_is_checked_on(O):
    """The GPU tests on the mixed matrix are void unless both classes occur: at least 8 tiles of each in the P = 1 slab and in both
    P = 2 slabs, and exactly the tiles the perturbation list names."""
    n = T.MIXED_N
    e = T.mixed_coo(O, n)
    rp, ci, va = csr_of(O, e, n)
    want = T.mixed_expected_class0(n)
    assert flipped(O, e, n) == want
    for world in (1, 2):
        for rank in range(world):
            off, nl = O.partition_rows(n * n, world, rank)
            cls, uniform, total = T.classify(rp, ci, va, n, off, nl)
            assert uniform >= 8 and total - uniform >= 8, (world, rank, uniform, total)
            assert total - uniform == len({(g, t) for g, t in want if off // n <= g < (off + nl) // n})


def test_the_two_lab_names_are_in_the_lab_build_only(B):
    product = open(B.LIB_PATH, "rb").read()
    lab = open(B.LAB_LIB_PATH, "rb").read()
    for name in (b"stream_coefficients", b"spmv_amd_cg_slab_tile_classes"):
        assert name not in product, name
        assert name in lab, name
    assert b"spmv_amd_cg_slab_uniform_tiles" in product
