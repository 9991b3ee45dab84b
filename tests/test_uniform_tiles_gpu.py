"""Uniform tiles of the CG slab's symmetric coefficient form (csrc/cg_slab_create.hip classify_tiles, csrc/spmv_kernels.hip rowlds_tile;
kernels.hpp SymPlanes): a row-lds tile whose coefficients all equal one slab-wide quintuple bit for bit loads no coefficient.
The class map must equal the numpy restatement (tests/tile_classes.py) exactly, and every result must be what the planes and the
CSR form compute, bit for bit."""
import numpy as np
import pytest

import tile_classes as T
from conftest import hist_err
from test_symmetric_coefficients_gpu import symmetric_coo


def slab_map(slab, n):
    cls = slab.tile_classes()
    return None if cls is None else cls.reshape(slab.n_local // n, T.col_tiles(n))


def check_map(slab, rp, ci, va, n):
    """The library's map and counts against the restatement; returns (uniform, total)."""
    want, uniform, total = T.classify(rp, ci, va, n, slab.row_offset, slab.n_local)
    got = slab_map(slab, n)
    assert slab.uniform_tiles() == (uniform, total)
    if want is None:
        assert got is None
    else:
        assert got is not None and got.shape == want.shape and np.array_equal(got, want)
    return uniform, total


def check_slabs(B, O, e, n, worlds, x, classes):
    """Every rank's slab of every split (staged communicator: spmv() fills the halos from the full vector): the map against the
    restatement, spmv() against the halo oracle bit for bit. classes(uniform, total, world, rank) asserts what the case expects."""
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    for world in worlds:
        for rank in range(world):
            comm = B.Comm.staged(rank, world, lambda *a: 0, lambda *a: 0) if world > 1 else None
            slab = B.CgSlab.from_matrix(m, comm)
            off, nl = O.partition_rows(n * n, world, rank)
            assert (slab.row_offset, slab.n_local) == (off, nl) and slab.coefficient_form() == 1
            classes(*check_map(slab, rp, ci, va, n), world, rank)
            base = rp[off]
            lrp = (rp[off:off + nl + 1] - base).astype(np.int32)
            hp = x[off - n:off] if rank > 0 else None
            hn = x[off + nl:off + nl + n] if rank < world - 1 else None
            want = O.spmv_halo(lrp, ci[base:], va[base:], x[off:off + nl], hp, hn, off, n * n, n)
            for stream in (0, 1, 0):
                slab.set_option("stream_coefficients", stream)
                assert np.array_equal(slab.spmv(x), want), (world, rank, stream)
            slab.destroy()
            if comm is not None:
                comm.destroy()


def all_uniform(uniform, total, world, rank):
    assert uniform == total > 0, (world, rank, uniform, total)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [640, 1000])
def test_generator_matrix_every_tile_uniform(Blab, O, n):
    """P = 1, 2, 4 slabs of the generator's matrix: uniform == total, the map equals the restatement, spmv() is the oracle's."""
    Blab.lib().spmv_amd_reset_host_matrices()
    x = np.random.default_rng(n).standard_normal(n * n)
    check_slabs(Blab, O, O.stencil5_coo(n), n, (1, 2, 4), x, all_uniform)
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3, 4])
def test_stand_in_slabs_every_tile_uniform(Blab, O, monkeypatch, P):
    """Every rank's slab of a P-GPU job at n = 3072 on one self-neighbour rank (boundary rows in the launch that waits for the halo
    and reduces): uniform == total, the map equals the restatement, and CG is bit-identical with the map ignored and in the CSR form."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_SELF_NEIGHBOUR", "1")
    n = 3072
    rp, ci, va = O.stencil5_csr(n)
    for r in range(P):
        comm = B.Comm.rccl(0, 1, B.Comm.unique_id())
        slab = B.CgSlab.stencil5_as(n, r, P, comm)
        assert slab.coefficient_form() == 1
        uniform, total = check_map(slab, rp, ci, va, n)
        assert uniform == total > 0, (P, r)
        ref = None
        for no_overlap in (0, 1):
            for stream, csr in ((0, 0), (1, 0), (0, 1)):
                slab.set_option("no_overlap", no_overlap)
                slab.set_option("stream_coefficients", stream)
                slab.set_option("csr_coefficients", csr)
                st = slab.solve(max_iters=9, tol=0.0)
                got = (st.iterations, slab.history().copy())
                if ref is None:
                    ref = got
                assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), (P, r, no_overlap, stream, csr)
        slab.destroy()
        comm.destroy()


@pytest.mark.gpu
def test_20k_slab_is_uniform_and_bit_identical_to_the_streaming_forms(Blab, golden):
    """The benchmark's slab: uniform == total > 0, 14 iterations on the golden history; history and gathered x bit-identical with the
    map ignored (stream_coefficients 1) and in the CSR form (csr_coefficients 1)."""
    g = golden["cases"].get("20000:5.0")
    if g is None:
        pytest.skip("20k golden not generated")
    n = 20000
    slab = Blab.CgSlab.stencil5(n)
    assert slab.coefficient_form() == 1 and slab.variant() == "stencil5/row-lds"
    uniform, total = slab.uniform_tiles()
    assert uniform == total == (n - 2) * T.col_tiles(n)
    st = slab.solve()
    h = slab.history().copy()
    assert st.iterations == g["cg"]["iterations"] == 14 and st.converged == 1
    assert hist_err(h, g["cg"]["history"]) < 1e-10
    x = slab.gather()
    for stream, csr in ((1, 0), (0, 1), (1, 1)):
        slab.set_option("stream_coefficients", stream)
        slab.set_option("csr_coefficients", csr)
        st2 = slab.solve()
        assert st2.iterations == 14 and np.array_equal(slab.history(), h), (stream, csr)
        assert np.array_equal(slab.gather(), x), (stream, csr)
    slab.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [640, 1000])
def test_random_symmetric_values_have_no_uniform_tile(Blab, O, n):
    """One random value per edge and per centre: no tile matches any quintuple; spmv() stays bit-exact against the halo oracle."""
    Blab.lib().spmv_amd_reset_host_matrices()
    rng = np.random.default_rng(n + 1)
    e = symmetric_coo(O, n, rng)
    x = rng.standard_normal(n * n)

    def none_uniform(uniform, total, world, rank):
        assert uniform == 0 and total > 0, (world, rank, uniform, total)

    check_slabs(Blab, O, e, n, (1, 2), x, none_uniform)
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_mixed_matrix_map_and_spmv(Blab, O):
    """The generator's matrix with perturbed edges and centres at the awkward places (tests/tile_classes.py, mixed_perturbations): the
    map equals the restatement exactly, both classes occur at least 8 times in every slab, spmv() is the halo oracle's."""
    Blab.lib().spmv_amd_reset_host_matrices()
    n = T.MIXED_N
    x = np.random.default_rng(3).standard_normal(n * n)

    def both(uniform, total, world, rank):
        assert uniform >= 8 and total - uniform >= 8, (world, rank, uniform, total)

    check_slabs(Blab, O, T.mixed_coo(O, n), n, (1, 2), x, both)
    Blab.lib().spmv_amd_reset_host_matrices()


def solve_all_forms(B, slab):
    """(iterations, verdict, history, x) under the map, with the map ignored, in the CSR form, and under the map again."""
    runs = []
    for stream, csr in ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0)):
        slab.set_option("stream_coefficients", stream)
        slab.set_option("csr_coefficients", csr)
        assert slab.coefficient_form() == 1 - csr
        st = slab.solve(max_iters=80, tol=1e-10)
        runs.append((st.iterations, st.converged, slab.history().copy(), slab.gather()))
    assert runs[0][1] == 1 and runs[0][0] > 10
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["1", "4", "16"])
@pytest.mark.parametrize("no_overlap", ["0", "1"])
def test_mixed_matrix_cg_bit_identical_across_forms(Blab, O, monkeypatch, ring, no_overlap):
    """CG on the mixed matrix, random right-hand side: iterations, history and gathered x are bit-identical under the class map, with
    the map ignored and in the CSR form, for ring lengths 1 / 4 / 16 and both loop shapes."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    monkeypatch.setenv("SPMV_AMD_NO_OVERLAP", no_overlap)
    n = T.MIXED_N
    m = B.HostMatrix(T.mixed_coo(O, n), n * n, n * n, n)
    slab = B.CgSlab.from_matrix(m)
    uniform, total = slab.uniform_tiles()
    assert uniform >= 8 and total - uniform >= 8
    slab.set_vectors(b=np.random.default_rng(17).standard_normal(n * n))
    solve_all_forms(B, slab)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["north_of_column_0", "west_of_last_column", "signed_zero", "one_ulp"])
def test_bits_that_differ_from_the_quintuple_cost_the_tile_its_class(Blab, O, kind):
    """A CSR holds no W in column 0 and no E in column n-1, so the exemption is tested from the other side: the N entry of column 0
    and the W entry of column n-1 are multiplied, and a change there makes the tile class 0. A -0.0 where the quintuple holds +0.0
    and a value 1 ulp off (both kept symmetric, so the planes stay) do the same; results stay bit-identical to the CSR form."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 640
    e = O.stencil5_coo(n)
    if kind == "north_of_column_0":
        T.set_edge(e, 40 * n, 39 * n, -1.5)
        want = {(40, 0), (39, 0)}
    elif kind == "west_of_last_column":
        T.set_edge(e, 80 * n + n - 1, 80 * n + n - 2, -1.5)
        want = {(80, T.col_tiles(n) - 1)}
    elif kind == "signed_zero":
        horizontal = np.abs(e["row"].astype(np.int64) - e["col"].astype(np.int64)) == 1
        e["value"][horizontal] = 0.0
        T.set_edge(e, 50 * n + 10, 50 * n + 11, -0.0)
        want = {(50, 0)}
    else:
        T.set_edge(e, 60 * n + 200, 61 * n + 200, np.nextafter(-1.0, 0.0))
        T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
        want = {(60, 1), (61, 1), (70, 1)}
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    slab = B.CgSlab.from_matrix(m)
    assert slab.coefficient_form() == 1
    uniform, total = check_map(slab, rp, ci, va, n)
    got = slab_map(slab, n)
    assert {(int(r), int(t)) for r, t in np.argwhere(got[1:n - 1] == 0) + [1, 0]} == want
    assert total - uniform == len(want)
    rng = np.random.default_rng(23)
    x = rng.standard_normal(n * n)
    y = slab.spmv(x)
    assert np.array_equal(y, O.spmv_stencil5(rp, ci, va, x, n))
    slab.set_option("csr_coefficients", 1)
    assert np.array_equal(slab.spmv(x), y)
    slab.set_option("csr_coefficients", 0)
    slab.set_vectors(b=rng.standard_normal(n * n))
    solve_all_forms(B, slab)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()
