"""The CG direction update inside the block SpMV (csrc/spmv_kernels.hip stencil5_direction_block_kernel and stencil5_block_list_kernel;
csrc/slab_decisions.hpp LoopShape::fused_direction): on a slab without neighbours the launch of iteration k + 1 evaluates p' = r + beta p on
its block tile and the two grid rows around it, stores its own rows and runs the block kernel's chains on the values it holds. Every
result must be what the two separate launches compute, bit for bit."""
import numpy as np
import pytest

import tile_classes as T

FUSED = "single rank: direction update inside the block SpMV"
BETA = 0.37


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def generator_slab(B, O, n, R):
    B.lib().spmv_amd_reset_host_matrices()
    e = O.stencil5_coo(n)
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    assert slab.coefficient_form() == 1 and slab.variant() == "stencil5/row-lds"
    slab.set_block_rows(R)
    return slab, O.build_csr(e, n * n)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", [640, 1000, 1003, 129, 130])
def test_the_fused_launch_alone_equals_the_two_launches_bit_for_bit(Blab, O, monkeypatch, n, R):
    """n = 640; 1000 (104 columns in the last tile); 1003 (odd: rows % 4 = rows % 8 = 3, grid rows not 16-byte aligned); 129 and 130
    forced onto row-lds (a last tile of one or two columns, rows % R = 1 or 2). p_out against r + beta * p in numpy (beta * p rounded,
    then added: the two roundings of fma(1.0, r, beta * p)), A p_out against the oracle, the partials and their sum against the in-loop
    SpMV of today on the same p_out; and a launch whose iteration does not match, or that finds the solve converged, writes nothing."""
    B = Blab
    if n < 512:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
    slab, (rp, ci, va) = generator_slab(B, O, n, R)
    rng = np.random.default_rng(1000 * n + R)
    r, p = rng.standard_normal(n * n), rng.standard_normal(n * n)
    p_out, Ap, partials, pAp = slab.direction_spmv(r, p, BETA)
    assert np.array_equal(bits(p_out), bits(r + BETA * p))
    assert np.array_equal(bits(Ap), bits(O.spmv_stencil5(rp, ci, va, p_out, n)))
    slab.set_option("fused_direction", 0)
    slab.set_option("spmv_with_dot", 1)
    assert np.array_equal(bits(slab.spmv(p_out)), bits(Ap))
    want_partials, want_pAp = slab.spmv_dot()
    assert len(partials) == len(want_partials) == n * T.col_tiles(n)
    assert np.array_equal(bits(partials), bits(want_partials))
    assert bits([pAp])[0] == bits([want_pAp])[0] and np.isfinite(pAp)
    slab.set_option("fused_direction", 1)
    for matches, converged in ((0, 0), (1, 1)):
        p_out, Ap, partials, pAp = slab.direction_spmv(r, p, BETA, iteration_matches=matches, converged=converged)
        assert np.isnan(p_out).all() and np.isnan(Ap).all() and np.isnan(partials).all(), (matches, converged)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["generator", "mixed"])
def test_the_slow_block_list_is_where_the_block_map_holds_0(Blab, O, matrix):
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 640 if matrix == "generator" else T.MIXED_N
    e = O.stencil5_coo(n) if matrix == "generator" else T.mixed_coo(O, n)
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    for R in (4, 8):
        slab.set_block_rows(R)
        for which in (0, 1):
            m = slab.block_map(which)
            got = slab.slow_blocks(which)
            assert got.dtype == np.int32 and np.array_equal(got, np.argwhere(m == 0).reshape(-1)), (R, which)
        row_blocks = n // R
        if matrix == "generator":  # the grid's first and last grid row sit in the first and the last row block
            assert len(slab.slow_blocks(0)) == 2 * T.col_tiles(n)
        else:
            assert len(slab.slow_blocks(0)) > 2 * T.col_tiles(n) and row_blocks > 2
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def solve_with_and_without(slab, option, **solve):
    """(iterations, verdict, history, x) with fused_direction 0, `option`, 0, and `option` twice in a row: all identical to the first."""
    runs, shapes = [], []
    for value in (0, option, 0, option, option):
        slab.set_option("fused_direction", value)
        shapes.append(slab.loop_shape())
        st = slab.solve(**solve)
        runs.append((st.iterations, st.converged, slab.history().copy(), slab.gather()))
    for k, r in enumerate(runs[1:]):
        assert r[:2] == runs[0][:2] and np.array_equal(bits(r[2]), bits(runs[0][2])) and np.array_equal(bits(r[3]), bits(runs[0][3])), k + 1
    return runs[0], shapes


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["4", "16"])
@pytest.mark.parametrize("matrix", ["generator_1003", "mixed"])
def test_whole_solves_are_bit_identical_with_the_direction_update_inside_the_spmv(Blab, O, monkeypatch, matrix, ring):
    """Random right-hand side; to convergence and five iterations at tol 0; ring 4 (more than four iterations: the window's flush runs
    before the fused launch, now a stage later, overwrites the slot) and 16; block_rows 4 and 8; run_ahead 2: every converging solve has
    one iteration enqueued past convergence, whose launches must return on the scalars."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    n = 1003 if matrix == "generator_1003" else T.MIXED_N
    e = O.stencil5_coo(n) if matrix == "generator_1003" else T.mixed_coo(O, n)
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    slab.set_vectors(b=np.random.default_rng(n + int(ring)).standard_normal(n * n))
    option = 1 if matrix == "generator_1003" else 2  # the mixed matrix: above the cap on the slow blocks' share or not, it runs fused
    for R in (4, 8):
        slab.set_block_rows(R)
        for run_ahead in (1, 2):
            slab.set_option("run_ahead", run_ahead)
            (iterations, converged, _, _), shapes = solve_with_and_without(slab, option, max_iters=80, tol=1e-10)
            assert converged == 1 and iterations > 10
            assert shapes == ["single rank", FUSED, "single rank", FUSED, FUSED]
            (iterations, converged, _, _), _ = solve_with_and_without(slab, option, max_iters=5, tol=0.0)
            assert (iterations, converged) == (5, 0)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("kind", ["north_of_column_0", "west_of_last_column", "signed_zero", "one_ulp"])
def test_a_perturbed_tile_goes_through_the_slow_list(Blab, O, kind, R):
    """The four "bits that differ from the quintuple" cases of test_block_rows_gpu.py at n = 640: the block with the class-0 tile only
    writes p' in the fused launch and is evaluated by the launch over the list."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 640
    e = O.stencil5_coo(n)
    if kind == "north_of_column_0":
        T.set_edge(e, 40 * n, 39 * n, -1.5)
        extra = 2 if 39 // R != 40 // R else 1
    elif kind == "west_of_last_column":
        T.set_edge(e, 80 * n + n - 1, 80 * n + n - 2, -1.5)
        extra = 1
    elif kind == "signed_zero":
        horizontal = np.abs(e["row"].astype(np.int64) - e["col"].astype(np.int64)) == 1
        e["value"][horizontal] = 0.0
        T.set_edge(e, 50 * n + 10, 50 * n + 11, -0.0)
        extra = 1
    else:
        T.set_edge(e, 60 * n + 200, 61 * n + 200, np.nextafter(-1.0, 0.0))
        T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
        extra = 2 if 60 // R == 61 // R else 3
    rp, ci, va = O.build_csr(e, n * n)
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    slab.set_block_rows(R)
    assert len(slab.slow_blocks(0)) == 2 * T.col_tiles(n) + extra
    rng = np.random.default_rng(29)
    r, p = rng.standard_normal(n * n), rng.standard_normal(n * n)
    p_out, Ap, _, _ = slab.direction_spmv(r, p, BETA)
    assert np.array_equal(bits(p_out), bits(r + BETA * p))
    assert np.array_equal(bits(Ap), bits(O.spmv_stencil5(rp, ci, va, p_out, n)))
    slab.set_vectors(b=rng.standard_normal(n * n))
    (iterations, converged, _, _), shapes = solve_with_and_without(slab, 1, max_iters=80, tol=1e-10)
    assert converged == 1 and iterations > 10 and shapes[1] == FUSED
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def one_solve(slab, **solve):
    st = slab.solve(**solve)
    return st.iterations, st.converged, slab.history().copy(), slab.gather()


def same(a, b):
    return a[:2] == b[:2] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3]))


@pytest.mark.gpu
def test_the_generator_matrix_on_one_rank_takes_the_fused_shape(Blab, O):
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    slab = B.CgSlab.stencil5(640)
    assert slab.loop_shape() == FUSED
    slab.set_block_rows(0)  # no block map: the one-row kernel and the direction update as a launch of its own
    assert slab.loop_shape() == "single rank"
    slab.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ring_1", "ring_1_no_overlap", "detailed_timers", "slow_share_above_the_cap"])
def test_a_slab_that_is_not_eligible_keeps_the_two_launches(Blab, O, monkeypatch, case):
    """Ring 1 (with SPMV_AMD_NO_OVERLAP either way), detailed timers, and a matrix whose slow blocks are more than 1 / 16 of its blocks
    under option 1: loop_shape() does not name the fused shape (detailed timers are a property of the solve: the shape it reports is
    the untimed solve's), and the solve equals option 0."""
    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    if case.startswith("ring_1"):
        monkeypatch.setenv("SPMV_AMD_P_RING", "1")
        monkeypatch.setenv("SPMV_AMD_NO_OVERLAP", "1" if case.endswith("no_overlap") else "0")
    n = 640
    e = O.stencil5_coo(n)
    if case == "slow_share_above_the_cap":
        # one perturbed centre in every 8th grid row of every column tile: 1/2 of the blocks of R = 4, all of R = 8
        for gi in range(4, n - 4, 8):
            for t in range(T.col_tiles(n)):
                T.set_entry(e, gi * n + 128 * t + 5, gi * n + 128 * t + 5, 5.5)
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    slab.set_vectors(b=np.random.default_rng(41).standard_normal(n * n))
    timers = 1 if case == "detailed_timers" else 0
    slab.set_option("fused_direction", 0)
    want = one_solve(slab, max_iters=80, tol=1e-10, timers=timers)
    slab.set_option("fused_direction", 1)
    if case == "detailed_timers":
        assert slab.loop_shape() == FUSED
    else:
        assert slab.loop_shape() == "single rank"
        if case == "slow_share_above_the_cap":
            assert 16 * len(slab.slow_blocks(0)) > len(slab.block_map(0))
    assert same(one_solve(slab, max_iters=80, tol=1e-10, timers=timers), want)
    if case == "detailed_timers":  # and the untimed fused solve agrees with both
        assert same(one_solve(slab, max_iters=80, tol=1e-10), want)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_a_slab_with_a_neighbour_keeps_its_shape(Blab, O):
    """World 2 over the staged transport, rank 0 of the split, in one process: the halo callback hands the slab its own last grid row
    back as the neighbour's (the slab mirrored at its cut), the all-reduce leaves the local sums -- a deterministic five-iteration
    solve. loop_shape() never names the fused shape and the solve does not depend on the option."""
    import ctypes as C

    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 640

    def mirror(user, send_prev, send_next, recv_prev, recv_next, count):
        if recv_next and send_next:
            C.memmove(recv_next, send_next, 8 * count)
        if recv_prev and send_prev:
            C.memmove(recv_prev, send_prev, 8 * count)
        return 0

    m = B.HostMatrix(O.stencil5_coo(n), n * n, n * n, n)
    comm = B.Comm.staged(0, 2, mirror, lambda *a: 0)
    slab = B.CgSlab.from_matrix(m, comm)
    slab.set_vectors(b=np.random.default_rng(43).standard_normal(n * n))
    runs = []
    for option in (0, 1, 2, 0):
        slab.set_option("fused_direction", option)
        assert "direction update inside" not in slab.loop_shape() and not slab.loop_shape().startswith("single rank")
        st = slab.solve(max_iters=5, tol=0.0)
        runs.append((st.iterations, st.converged, slab.history().copy(), None))
    assert runs[0][0] == 5 and np.isfinite(runs[0][2]).all()
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and np.array_equal(bits(r[2]), bits(runs[0][2]))
    with pytest.raises(RuntimeError):
        slab.direction_spmv(np.zeros(slab.n_local), np.zeros(slab.n_local), BETA)
    slab.destroy()
    comm.destroy()
    B.lib().spmv_amd_reset_host_matrices()
