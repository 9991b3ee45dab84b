"""Block tiles of the CG slab's in-loop SpMV (csrc/spmv_kernels.hip stencil5_rowlds_block_kernel; csrc/cg_slab_create.hip build_block_maps;
kernels.hpp Stencil5Plan): one wave evaluates 128 columns x R grid rows, R = 4 or 8. The block maps must equal the numpy restatement
(tests/block_map.py) exactly, and every result must be what block_rows = 0 -- the one-row kernel -- computes, bit for bit."""
import numpy as np
import pytest

import block_map as K
import tile_classes as T
from test_uniform_tiles_gpu import solve_all_forms

SETTINGS = (0, 4, 8, 0)  # block_rows in turn, on the same slab: ends where it started


def slab_of(B, m, world, rank):
    comm = B.Comm.staged(rank, world, lambda *a: 0, lambda *a: 0) if world > 1 else None
    return B.CgSlab.from_matrix(m, comm), comm


def restated_classes(rp, ci, va, n, slab):
    """The class map the library keeps for this slab, restated (None: the slab is not made of whole grid rows and keeps no map)."""
    if slab.row_offset % n != 0 or slab.n_local % n != 0:
        return None
    return T.classify(rp, ci, va, n, slab.row_offset, slab.n_local)[0]


def check_block_maps(slab, cls, n, world, rank, seen):
    """Both ranges' maps against the restatement for R = 4, 8 and 0; adds (R, row count % R) of every range that has a map to `seen`."""
    rows = slab.n_local // n
    for R in (4, 8, 0, 8):
        slab.set_block_rows(R)
        for which, (lo, hi) in enumerate(K.launch_ranges(rows, rank > 0, rank < world - 1)):
            want = K.block_map(cls, lo, hi, R)
            got = slab.block_map(which)
            if want is None:
                assert got is None, (world, rank, R, which)
            else:
                assert got is not None and np.array_equal(got, want.reshape(-1)), (world, rank, R, which)
                seen.add((R, (hi - lo) % R))


@pytest.mark.gpu
def test_block_maps_equal_the_restatement_on_the_generator_matrix(Blab, O):
    """n = 640 and n = 1000, worlds 1, 2, 3 and 4 (world 3 cuts inside grid rows: no class map, no block map). World 4 is there for
    its interior ranges of 249 grid rows at n = 1000: with 640, 320, 319, 1000, 500 and 499 alone no range leaves remainder 1."""
    B = Blab
    seen = set()
    for n in (640, 1000):
        B.lib().spmv_amd_reset_host_matrices()
        e = O.stencil5_coo(n)
        rp, ci, va = O.build_csr(e, n * n)
        m = B.HostMatrix(e, n * n, n * n, n)
        for world in (1, 2, 3, 4):
            for rank in range(world):
                slab, comm = slab_of(B, m, world, rank)
                assert (slab.row_offset, slab.n_local) == O.partition_rows(n * n, world, rank)
                cls = restated_classes(rp, ci, va, n, slab)
                assert (cls is None) == (world == 3)
                check_block_maps(slab, cls, n, world, rank, seen)
                slab.destroy()
                if comm is not None:
                    comm.destroy()
    B.lib().spmv_amd_reset_host_matrices()
    for R in K.BLOCK_ROWS:
        assert {(R, 0), (R, 1), (R, R - 1)} <= seen, (R, sorted(seen))


@pytest.mark.gpu
def test_block_maps_equal_the_restatement_on_the_mixed_matrix(Blab, O):
    """Both classes in every slab: blocks with a class-0 tile in any of their rows are slow, in both ranges."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = T.MIXED_N
    e = T.mixed_coo(O, n)
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    seen = set()
    for world in (1, 2):
        for rank in range(world):
            slab, comm = slab_of(B, m, world, rank)
            cls = restated_classes(rp, ci, va, n, slab)
            assert cls is not None and (cls[1:-1] == 0).any()
            check_block_maps(slab, cls, n, world, rank, seen)
            for R in K.BLOCK_ROWS:  # slow blocks other than the first and the last of the whole range
                assert (K.block_map(cls, 0, cls.shape[0], R)[1:-1] == 0).any()
            slab.destroy()
            if comm is not None:
                comm.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def check_spmv(B, O, e, n, worlds, x):
    """spmv() of every rank's slab against the halo oracle for block_rows 0, 4, 8, 0 in turn: as a plain y = A x (the one-row kernel
    whatever block_rows is) and in its in-loop form (spmv_with_dot: the block kernel over the whole slab or over the interior rows,
    the boundary rows in the launch that reduces)."""
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    for world in worlds:
        for rank in range(world):
            slab, comm = slab_of(B, m, world, rank)
            off, nl = slab.row_offset, slab.n_local
            assert slab.coefficient_form() == 1 and slab.variant() == "stencil5/row-lds"
            base = rp[off]
            lrp = (rp[off:off + nl + 1] - base).astype(np.int32)
            hp = x[off - n:off] if rank > 0 else None
            hn = x[off + nl:off + nl + n] if rank < world - 1 else None
            want = O.spmv_halo(lrp, ci[base:], va[base:], x[off:off + nl], hp, hn, off, n * n, n)
            for R in SETTINGS:
                slab.set_block_rows(R)
                assert (slab.block_map(0) is not None) == (R > 0)
                for with_dot in (1, 0):
                    slab.set_option("spmv_with_dot", with_dot)
                    assert np.array_equal(slab.spmv(x), want), (n, world, rank, R, with_dot)
            slab.destroy()
            if comm is not None:
                comm.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["generator", "mixed"])
def test_spmv_bit_exact_for_every_block_rows(Blab, O, matrix):
    """n = 1000 (104 columns in the last tile; 1000, 500, 499, 250, 249, 248 rows per range) on the generator's matrix, and the mixed
    matrix (fast and slow blocks side by side), P = 1, 2 and 4."""
    Blab.lib().spmv_amd_reset_host_matrices()
    n = 1000 if matrix == "generator" else T.MIXED_N
    e = O.stencil5_coo(n) if matrix == "generator" else T.mixed_coo(O, n)
    x = np.random.default_rng(n + 5).standard_normal(n * n)
    check_spmv(Blab, O, e, n, (1, 2, 4), x)
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 130])
def test_spmv_bit_exact_on_a_small_grid_with_a_last_tile_of_one_or_two_columns(Blab, O, monkeypatch, n):
    """A grid below 512 forced onto row-lds: the second tile holds one column (n = 129) or two (n = 130)."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
    Blab.lib().spmv_amd_reset_host_matrices()
    x = np.random.default_rng(n).standard_normal(n * n)
    check_spmv(Blab, O, O.stencil5_coo(n), n, (1,), x)
    Blab.lib().spmv_amd_reset_host_matrices()


def solve_for_every_block_rows(slab, **solve):
    """(iterations, verdict, history, x) for block_rows 0, 4, 8, 0: all identical to the first."""
    runs = []
    for R in SETTINGS:
        slab.set_block_rows(R)
        st = slab.solve(**solve)
        runs.append((st.iterations, st.converged, slab.history().copy(), slab.gather()))
    for R, r in zip(SETTINGS[1:], runs[1:]):
        assert r[:2] == runs[0][:2] and np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3]), R
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["1", "4", "16"])
@pytest.mark.parametrize("no_overlap", ["0", "1"])
def test_mixed_matrix_cg_bit_identical_for_every_block_rows(Blab, O, monkeypatch, ring, no_overlap):
    """CG on the mixed matrix, random right-hand side, to convergence: reversed sweeps, every partial slot, and the launch enqueued
    past convergence (the skip flag) -- for ring lengths 1 / 4 / 16 and both loop shapes."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    monkeypatch.setenv("SPMV_AMD_NO_OVERLAP", no_overlap)
    n = T.MIXED_N
    m = B.HostMatrix(T.mixed_coo(O, n), n * n, n * n, n)
    slab = B.CgSlab.from_matrix(m)
    slab.set_vectors(b=np.random.default_rng(17).standard_normal(n * n))
    iterations, converged, _, _ = solve_for_every_block_rows(slab, max_iters=80, tol=1e-10)
    assert converged == 1 and iterations > 10
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3, 4])
def test_stand_in_slabs_cg_bit_identical_for_every_block_rows(Blab, monkeypatch, P):
    """Every rank's slab of a P-GPU job at n = 3072 on one self-neighbour rank: the block kernel over the interior rows, the boundary
    rows in the launch that waits for the halo and reduces; 9 iterations, both loop shapes."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_SELF_NEIGHBOUR", "1")
    n = 3072
    for r in range(P):
        comm = B.Comm.rccl(0, 1, B.Comm.unique_id())
        slab = B.CgSlab.stencil5_as(n, r, P, comm)
        assert slab.coefficient_form() == 1
        ref = None
        for no_overlap in (0, 1):
            slab.set_option("no_overlap", no_overlap)
            got = solve_for_every_block_rows(slab, max_iters=9, tol=0.0)
            if ref is None:
                ref = got
            assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), (P, r, no_overlap)
        slab.destroy()
        comm.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("R", K.BLOCK_ROWS)
@pytest.mark.parametrize("kind", ["north_of_column_0", "west_of_last_column", "signed_zero", "one_ulp"])
def test_a_block_with_a_perturbed_tile_takes_the_row_by_row_path(Blab, O, kind, R):
    """The four "bits that differ from the quintuple" cases at n = 640: the block that holds the class-0 tile is slow in the map, and
    spmv() and CG equal the CSR form bit for bit."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 640
    e = O.stencil5_coo(n)
    if kind == "north_of_column_0":
        T.set_edge(e, 40 * n, 39 * n, -1.5)
        tiles = {(40, 0), (39, 0)}
    elif kind == "west_of_last_column":
        T.set_edge(e, 80 * n + n - 1, 80 * n + n - 2, -1.5)
        tiles = {(80, T.col_tiles(n) - 1)}
    elif kind == "signed_zero":
        horizontal = np.abs(e["row"].astype(np.int64) - e["col"].astype(np.int64)) == 1
        e["value"][horizontal] = 0.0
        T.set_edge(e, 50 * n + 10, 50 * n + 11, -0.0)
        tiles = {(50, 0)}
    else:
        T.set_edge(e, 60 * n + 200, 61 * n + 200, np.nextafter(-1.0, 0.0))
        T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
        tiles = {(60, 1), (61, 1), (70, 1)}
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    slab = B.CgSlab.from_matrix(m)
    assert slab.coefficient_form() == 1
    slab.set_block_rows(R)
    got = slab.block_map(0).reshape(-1, T.col_tiles(n))
    blocks = got.shape[0]
    slow = {(int(b), int(t)) for b, t in np.argwhere(got[1:blocks - 1] == 0) + [1, 0]}
    assert slow == {(gi // R, t) for gi, t in tiles} and not got[0].any() and not got[blocks - 1].any()
    rng = np.random.default_rng(23)
    x = rng.standard_normal(n * n)
    slab.set_option("spmv_with_dot", 1)
    y = slab.spmv(x)
    assert np.array_equal(y, O.spmv_stencil5(rp, ci, va, x, n))
    slab.set_option("csr_coefficients", 1)
    assert np.array_equal(slab.spmv(x), y)
    slab.set_option("csr_coefficients", 0)
    slab.set_vectors(b=rng.standard_normal(n * n))
    solve_all_forms(B, slab)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()
