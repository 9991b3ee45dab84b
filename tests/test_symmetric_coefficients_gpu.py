"""The symmetric coefficient form of the CG slab (csrc/cg_slab.hpp, kernels.hpp SymPlanes): a slab whose W / N entries equal, bit
for bit, the E entry of row i-1 / the S entry of row i-n streams [C, E] + S planes (24 B/row) instead of its CSR values (40 B/row).
Results must be the CSR form's, bit for bit; any matrix that is not bitwise symmetric keeps the CSR form."""
import numpy as np
import pytest

from conftest import hist_err


def symmetric_coo(O, n, rng):
    """The n x n 5-point pattern with one random value per undirected edge and a random centre (diagonally dominant: SPD)."""
    e = O.stencil5_coo(n)
    r, c = e["row"].astype(np.int64), e["col"].astype(np.int64)
    key = np.minimum(r, c) * (n * n) + np.maximum(r, c)
    uniq, inv = np.unique(key, return_inverse=True)
    vals = rng.uniform(-1.2, -0.8, len(uniq))[inv]
    diag = r == c
    vals[diag] = rng.uniform(4.9, 5.1, int(diag.sum()))
    e["value"] = vals
    return e


def entry(e, row, col):
    return int(np.flatnonzero((e["row"] == row) & (e["col"] == col))[0])


def check_slabs(B, O, e, n, worlds, x, want_form):
    """slab.spmv of every rank of every split against the halo oracle, bit for bit; want_form(world, off, nl) -> expected form."""
    rp, ci, va = O.build_csr(e, n * n)
    m = B.HostMatrix(e, n * n, n * n, n)
    for world in worlds:
        for rank in range(world):
            comm = B.Comm.staged(rank, world, lambda *a: 0, lambda *a: 0) if world > 1 else None
            slab = B.CgSlab.from_matrix(m, comm)
            off, nl = O.partition_rows(n * n, world, rank)
            assert (slab.row_offset, slab.n_local) == (off, nl)
            assert slab.coefficient_form() == want_form(world, off, nl), (world, rank)
            base = rp[off]
            lrp = (rp[off:off + nl + 1] - base).astype(np.int32)
            hp = x[off - n:off] if rank > 0 else None
            hn = x[off + nl:off + nl + n] if rank < world - 1 else None
            want = O.spmv_halo(lrp, ci[base:], va[base:], x[off:off + nl], hp, hn, off, n * n, n)
            assert np.array_equal(slab.spmv(x), want), (world, rank)
            slab.destroy()
            if comm is not None:
                comm.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,rowlds_min_grid", [(130, "2"), (260, "2"), (640, None), (1000, None)])
def test_planes_slab_spmv_bit_exact_against_halo_oracle(B, O, fresh_host_matrices, monkeypatch, n, rowlds_min_grid):
    """P = 1, 2, 4 slabs on one GPU (staged communicator: spmv() fills the halos from the full vector), random symmetric values.
    Slabs of whole grid rows take the planes; the others (130 rows over 4 ranks) run row-generic on the CSR."""
    if rowlds_min_grid is not None:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", rowlds_min_grid)
    rng = np.random.default_rng(n)
    e = symmetric_coo(O, n, rng)
    x = rng.standard_normal(n * n)
    check_slabs(B, O, e, n, (1, 2, 4), x, lambda world, off, nl: 1 if n % world == 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["w_ulp", "n_ulp", "signed_zero"])
def test_bits_that_are_not_symmetric_keep_the_csr_form(B, O, fresh_host_matrices, kind):
    """One W entry 1 ulp off its partner, one N entry 1 ulp off, or a -0.0 / +0.0 pair (equal under ==, not as bits): the slab
    that owns the row keeps the CSR form and computes what the CSR path computes; slabs without the row are unaffected."""
    n = 640
    rng = np.random.default_rng(5)
    e = symmetric_coo(O, n, rng)
    i = 100 * n + 200  # interior row of the first half
    if kind == "w_ulp":
        k = entry(e, i, i - 1)
        e["value"][k] = np.nextafter(e["value"][k], 0.0)
    elif kind == "n_ulp":
        k = entry(e, i, i - n)
        e["value"][k] = np.nextafter(e["value"][k], -np.inf)
    else:
        e["value"][entry(e, i, i - 1)] = -0.0
        e["value"][entry(e, i - 1, i)] = 0.0
    x = rng.standard_normal(n * n)
    check_slabs(B, O, e, n, (1, 2), x, lambda world, off, nl: 0 if off <= i < off + nl else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["1", "4", "16"])
@pytest.mark.parametrize("no_overlap", ["0", "1"])
def test_cg_planes_and_csr_form_bit_identical_single_rank(Blab, O, monkeypatch, ring, no_overlap):
    """Random symmetric SPD matrix, random right-hand side: iterations, residual history and gathered x of the planes and of the
    CSR form (LAB option csr_coefficients) are bit-identical, for ring lengths 1 / 4 / 16 and both loop shapes."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    monkeypatch.setenv("SPMV_AMD_NO_OVERLAP", no_overlap)
    n = 640
    rng = np.random.default_rng(11)
    e = symmetric_coo(O, n, rng)
    m = B.HostMatrix(e, n * n, n * n, n)
    slab = B.CgSlab.from_matrix(m)
    slab.set_vectors(b=rng.standard_normal(n * n))
    runs = []
    for csr in (0, 1, 0):
        slab.set_option("csr_coefficients", csr)
        assert slab.coefficient_form() == 1 - csr
        st = slab.solve(max_iters=80, tol=1e-10)
        runs.append((st.iterations, st.converged, slab.history().copy(), slab.gather()))
    assert runs[0][1] == 1 and runs[0][0] > 10
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3, 4])
def test_cg_planes_on_stand_in_slabs_with_halos(Blab, monkeypatch, P):
    """Every rank's slab of a P-GPU job on one self-neighbour rank (halos on both sides where the rank has neighbours: the
    boundary rows run in the launch that waits for the halo's arrival flag and reduces the partials). Planes and CSR form give
    the same iterations and history, bit for bit, for ring lengths 1 / 4 / 16 and both loop shapes."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_SELF_NEIGHBOUR", "1")
    n = 3072  # whole grid rows per slab for P = 2, 3, 4
    for ring in ("16", "4", "1"):
        monkeypatch.setenv("SPMV_AMD_P_RING", ring)
        for r in range(P):
            comm = B.Comm.rccl(0, 1, B.Comm.unique_id())
            slab = B.CgSlab.stencil5_as(n, r, P, comm)
            assert slab.coefficient_form() == 1
            kw = dict(max_iters=9, tol=0.0)
            ref = None
            for no_overlap in (0, 1):
                for csr in (1, 0):
                    slab.set_option("no_overlap", no_overlap)
                    slab.set_option("csr_coefficients", csr)
                    st = slab.solve(**kw)
                    got = (st.iterations, slab.history().copy())
                    if ref is None:
                        ref = got
                    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), (ring, r, no_overlap, csr)
            slab.destroy()
            comm.destroy()


@pytest.mark.gpu
def test_cg_20k_slab_takes_the_planes_and_matches_golden(Blab, golden):
    """The generator's 20 000^2 slab (the benchmark's) streams the planes, converges in 14 iterations on the committed golden
    history, and its history is bit-identical to the CSR form's."""
    g = golden["cases"].get("20000:5.0")
    if g is None:
        pytest.skip("20k golden not generated")
    slab = Blab.CgSlab.stencil5(20000)
    assert slab.coefficient_form() == 1 and slab.variant() == "stencil5/row-lds"
    st = slab.solve()
    h = slab.history().copy()
    assert st.iterations == g["cg"]["iterations"] == 14 and st.converged == 1
    assert hist_err(h, g["cg"]["history"]) < 1e-10
    slab.set_option("csr_coefficients", 1)
    st2 = slab.solve()
    assert st2.iterations == 14 and np.array_equal(slab.history(), h)
    slab.destroy()


def test_csr_form_option_exists_in_the_lab_build_only(B):
    """The option that forces the CSR form is a LAB-build hook: its name is compiled into libspmv_amd_lab.so only."""
    product = open(B.LIB_PATH, "rb").read()
    lab = open(B.LAB_LIB_PATH, "rb").read()
    assert b"csr_coefficients" not in product
    assert b"csr_coefficients" in lab
