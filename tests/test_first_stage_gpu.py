"""b serves as p0 (csrc/slab_decisions.hpp LoopShape::b_is_p0; csrc/spmv_kernels.hip stencil5_first_block_kernel): on a slab without
neighbours that owns its matrix, with x0 the library's zeros and a matrix whose every row sums to +0.0 over zero operands, r0 = b - A 0
is b bit for bit. A solve then enqueues no launch for r0: iteration 0's block SpMV goes first, on b, and sums b.b beside b.(A b); b is
read wherever the first window reads ring slot 0 and is never written. Every result must be what the launches of before compute
(set_option("zero_start_parts", 7): the launch that stores r0 = b as p0 and sums r0.r0, then the block SpMV on it), bit for bit."""
import numpy as np
import pytest

import tile_classes as T
from test_zero_start_gpu import bits, one_solve, rhs, same, slab_of

ZERO_X, R0_ONCE = 1, 2  # bits of CgSlab.initial_form(); CgSlab.first_form() is the shape of this file
POISON = 0xFFFFFFFFFFFFFFFF


def rhs_with_subnormals(n, seed):
    """test_zero_start_gpu.rhs (random, with +0.0 and -0.0 in the corners, on both edge columns and inside) and subnormals of both
    signs: their squares underflow to zero in b.b and their products with the coefficients stay subnormal in A b."""
    b = rhs(n, seed)
    spots = np.random.default_rng(seed + 1).integers(0, n * n, 24)
    b[spots[0::2]] = 4.9e-324
    b[spots[1::2]] = -2.5e-310
    b[n + 1], b[n * n - 2] = 2.2250738585072009e-308, -4.9e-324  # the largest subnormal; one in the grid's last grid row
    return b


def launches_of_before(slab, b, R):
    """(A b, p.Ap partials, pAp, r0.r0 partials, rr) by the launches a solve with zero_start_parts 7 enqueues: the first launch of the
    zero start through the initial stage (r0 stored once as p0: it must BE b), then the in-loop SpMV of block_rows R on it."""
    slab.set_option("zero_start_parts", 7)
    assert slab.first_form() == 0
    form, r0, _, rr_partials, rr = slab.initial_stage()
    assert form == ZERO_X | R0_ONCE and np.array_equal(bits(r0), bits(b))
    slab.set_block_rows(R)
    slab.set_option("spmv_with_dot", 1)
    Ap = slab.spmv(r0)
    partials, pAp = slab.spmv_dot()
    slab.set_option("spmv_with_dot", 0)
    slab.set_option("zero_start_parts", 15)
    return Ap, partials, pAp, rr_partials, rr


def first_stage_equals(slab, want, n, b):
    """The first stage in both sweep directions against launches_of_before's tuple: every array and both sums as uint64; every slot
    of both (poisoned) partial arrays was written, and the arrays hold exactly the plan's slots."""
    want_Ap, want_partials, want_pAp, want_rr_partials, want_rr = want
    assert slab.first_form() == 1
    for reverse in (True, False):
        Ap, partials, bb_partials, rr, pAp = slab.first_stage(reverse=reverse)
        assert len(partials) == len(bb_partials) == len(want_partials) == len(want_rr_partials) == n * T.col_tiles(n)
        assert not (bits(partials) == POISON).any() and not (bits(bb_partials) == POISON).any() and not (bits(Ap) == POISON).any()
        assert np.array_equal(bits(Ap), bits(want_Ap)), reverse
        assert np.array_equal(bits(partials), bits(want_partials)), reverse
        assert np.array_equal(bits(bb_partials), bits(want_rr_partials)), reverse
        assert bits([rr])[0] == bits([want_rr])[0] and bits([pAp])[0] == bits([want_pAp])[0], reverse
        assert np.isfinite(rr) and rr > 0 and np.isfinite(pAp)
    assert np.array_equal(bits(slab.stored_b()), bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", [129, 130, 192, 193, 640, 1003])
def test_the_first_stage_alone_equals_the_two_launches_bit_for_bit(Blab, O, monkeypatch, n, R):
    """Last column tile of 1 (129), 2 (130), 64 (192), 65 (193) and 128 (640) columns and of 107 at the odd 1003; grid-row counts that
    are 1, 2, 0, 1, 0 and 3 mod 4 and 1, 2, 0, 1, 0 and 3 mod 8 (a short last block in all but two). b random with signed zeros and
    subnormals. A b also against the oracle."""
    B = Blab
    if n < 512:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
    e = O.stencil5_coo(n)
    slab = slab_of(B, e, n)
    b = rhs_with_subnormals(n, 31 * n + R)
    slab.set_vectors(b=b)
    want = launches_of_before(slab, b, R)
    rp, ci, va = O.build_csr(e, n * n)
    assert np.array_equal(bits(want[0]), bits(O.spmv_stencil5(rp, ci, va, b, n)))
    first_stage_equals(slab, want, n, b)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def perturbed(O, kind, n):
    """The "mixed" matrix of tile_classes.py, or one of test_fused_direction_gpu.py's four matrices with a tile whose bits differ from
    the quintuple."""
    if kind == "mixed":
        return T.mixed_coo(O, n)
    e = O.stencil5_coo(n)
    if kind == "north_of_column_0":
        T.set_edge(e, 40 * n, 39 * n, -1.5)
    elif kind == "west_of_last_column":
        T.set_edge(e, 80 * n + n - 1, 80 * n + n - 2, -1.5)
    elif kind == "signed_zero":
        horizontal = np.abs(e["row"].astype(np.int64) - e["col"].astype(np.int64)) == 1
        e["value"][horizontal] = 0.0
        T.set_edge(e, 50 * n + 10, 50 * n + 11, -0.0)
    else:
        assert kind == "one_ulp"
        T.set_edge(e, 60 * n + 200, 61 * n + 200, np.nextafter(-1.0, 0.0))
        T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed", "north_of_column_0", "west_of_last_column", "signed_zero", "one_ulp"])
def test_blocks_that_are_not_fast_go_row_by_row_with_both_partials(Blab, O, kind):
    """n = 640, R = 4 and 8: the blocks whose map byte is 0 -- a class-0 tile inside, the grid's first and last grid row -- emit, row
    by row, the partials the ONE-ROW kernels give: the reference here is block_rows 0 (stencil5_rowlds_kernel<1>) and the initial
    stage's one-row launch. Checked on the whole arrays and, named, on the slots of the rows that lie in map-0 blocks."""
    B = Blab
    n = T.MIXED_N
    slab = slab_of(B, perturbed(O, kind, n), n)
    b = rhs_with_subnormals(n, 7)
    slab.set_vectors(b=b)
    want = launches_of_before(slab, b, 0)
    ct = T.col_tiles(n)
    for R in (4, 8):
        slab.set_block_rows(R)
        m = np.asarray(slab.block_map(0)).reshape(-1, ct)
        assert len(slab.slow_blocks(0)) > 2 * ct  # more than the grid's first and last grid row
        first_stage_equals(slab, want, n, b)
        _, partials, bb_partials, _, _ = slab.first_stage()
        slow_rows = np.repeat(m == 0, R, axis=0)[:n].reshape(-1)  # slot (grid row, column tile) -> its block is not fast
        assert slow_rows.sum() == R * len(slab.slow_blocks(0))  # 640 grid rows: no short block
        assert np.array_equal(bits(partials)[slow_rows], bits(want[1])[slow_rows])
        assert np.array_equal(bits(bb_partials)[slow_rows], bits(want[3])[slow_rows])
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def solve_each_way(slab, b, **solve):
    """(iterations, verdict, history, x) with zero_start_parts 7, 15, 7, 15, 15 and with zero_start 0: all identical to the first; b on
    the device is what was uploaded after every one of them."""
    runs = []
    for parts in (7, 15, 7, 15, 15, None):
        slab.set_option("zero_start", 0 if parts is None else 1)
        if parts is not None:
            slab.set_option("zero_start_parts", parts)
            assert slab.first_form() == (1 if parts == 15 else 0)
        runs.append(one_solve(slab, **solve))
        assert np.array_equal(bits(slab.stored_b()), bits(b)), (parts, solve)
    slab.set_option("zero_start", 1)
    slab.set_option("zero_start_parts", 15)
    for k, r in enumerate(runs[1:]):
        assert same(r, runs[0]), (k + 1, solve)
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["2", "4", "16"])
@pytest.mark.parametrize("matrix", ["generator_1003", "mixed"])
def test_whole_solves_are_bit_identical_with_b_as_p0(Blab, O, monkeypatch, matrix, ring):
    """Rings 2, 4 and 16 with more iterations than the ring (the real slot 0 is written when the ring wraps, behind the flush that read
    b in its place), run_ahead 0 and 2, fused_direction 0 and 1 (2 on the mixed matrix), block_rows 4 and 8: to convergence, five
    iterations at tol 0 (ring 4: the window is flushed once with b in it), one iteration, none (x = x0, the history's one entry), and a
    tolerance the first iteration meets. Then another b on the same slab: its own results, nothing of the first b is kept."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    n = 1003 if matrix == "generator_1003" else T.MIXED_N
    e = O.stencil5_coo(n) if matrix == "generator_1003" else T.mixed_coo(O, n)
    slab = slab_of(B, e, n)
    b = rhs_with_subnormals(n, n + int(ring))
    slab.set_vectors(b=b)
    fused = 1 if matrix == "generator_1003" else 2
    for k, (R, direction, run_ahead) in enumerate([(4, fused, 0), (8, 0, 2), (4, 0, 0), (8, fused, 2)]):
        slab.set_block_rows(R)
        slab.set_option("fused_direction", direction)
        slab.set_option("run_ahead", run_ahead)
        iterations, converged, _, _ = solve_each_way(slab, b, max_iters=80, tol=1e-10)
        assert converged == 1 and iterations > 16
        assert solve_each_way(slab, b, max_iters=5, tol=0.0)[:2] == (5, 0)
        if k == 0:
            assert solve_each_way(slab, b, max_iters=1, tol=0.0)[:2] == (1, 0)
            none = solve_each_way(slab, b, max_iters=0, tol=0.0)
            assert none[0] == 0 and len(none[2]) == 1 and np.array_equal(bits(none[3]), bits(np.zeros(n * n)))
            assert solve_each_way(slab, b, max_iters=80, tol=0.9)[:2] == (1, 1)
            assert solve_each_way(slab, b, timeline=True, max_iters=80, tol=1e-10)[:2] == (iterations, 1)
    first = one_solve(slab, max_iters=80, tol=1e-10)
    other = rhs_with_subnormals(n, 99)
    slab.set_vectors(b=other)
    second = solve_each_way(slab, other, max_iters=80, tol=1e-10)
    assert not np.array_equal(bits(first[3]), bits(second[3]))
    fresh = slab_of(B, e, n)
    fresh.set_block_rows(8)
    fresh.set_option("fused_direction", fused)
    fresh.set_option("run_ahead", 2)
    fresh.set_option("zero_start", 0)
    fresh.set_vectors(b=other)
    assert same(one_solve(fresh, max_iters=80, tol=1e-10), second)
    fresh.destroy()
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def five_iterations_equal_parts_7(slab):
    """Under zero_start_parts 15 the slab reports no b-as-p0 shape, and five iterations equal zero_start_parts 7's bit for bit."""
    slab.set_option("zero_start_parts", 15)
    assert slab.first_form() == 0
    with pytest.raises(RuntimeError):
        slab.first_stage()
    got = one_solve(slab, max_iters=5, tol=0.0)
    slab.set_option("zero_start_parts", 7)
    assert slab.first_form() == 0
    assert same(one_solve(slab, max_iters=5, tol=0.0), got) and got[0] == 5
    slab.set_option("zero_start_parts", 15)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["all_negative_row", "minus_zero_row", "infinite_coefficient", "uploaded_x0", "ring_1"])
def test_the_gate_on_one_rank(Blab, O, monkeypatch, case):
    """One row whose five coefficients are all negative (A 0 = -0.0 there: b = -0.0 would come out as +0.0); one row that stores -0.0
    only; an infinite coefficient (the shape alone: no solve); an x0 the caller uploaded, all zeros; ring 1. None takes the shape, and
    each solves as zero_start_parts 7 does. The first three keep the zero start's other parts: only the matrix fact is missing."""
    B = Blab
    n = 640
    e = O.stencil5_coo(n)
    hot = 200 * n + 300
    if case == "all_negative_row":
        T.set_entry(e, hot, hot, -5.0)
    elif case == "minus_zero_row":
        T.set_entry(e, hot, hot, -0.0)
        for other in (hot - 1, hot + 1, hot - n, hot + n):
            T.set_edge(e, hot, other, -0.0)
    elif case == "infinite_coefficient":
        T.set_entry(e, hot, hot, np.inf)
    elif case == "ring_1":
        monkeypatch.setenv("SPMV_AMD_P_RING", "1")
    slab = slab_of(B, e, n)
    b = rhs_with_subnormals(n, 3)
    b[hot] = -0.0  # where a wrong A 0 would show
    slab.set_vectors(b=b)
    if case == "uploaded_x0":
        assert slab.first_form() == 1
        slab.set_vectors(x0=np.zeros(n * n))
        assert slab.initial_form() == R0_ONCE
    elif case == "ring_1":
        assert slab.initial_form() == 0
    else:
        assert slab.initial_form() == ZERO_X | R0_ONCE
    if case == "infinite_coefficient":
        assert slab.first_form() == 0
    else:
        five_iterations_equal_parts_7(slab)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_the_gate_on_a_slab_with_a_neighbour(Blab, O):
    """World 2 over the staged transport, rank 0 of the split at n = 512, in one process (the halo callback mirrors the slab at its
    cut, as in test_fused_direction_gpu.py): never the shape, and the solve does not depend on the part bit."""
    import ctypes as C

    B = Blab
    B.lib().spmv_amd_reset_host_matrices()
    n = 512

    def mirror(user, send_prev, send_next, recv_prev, recv_next, count):
        if recv_next and send_next:
            C.memmove(recv_next, send_next, 8 * count)
        if recv_prev and send_prev:
            C.memmove(recv_prev, send_prev, 8 * count)
        return 0

    comm = B.Comm.staged(0, 2, mirror, lambda *a: 0)
    slab = B.CgSlab.from_matrix(B.HostMatrix(O.stencil5_coo(n), n * n, n * n, n), comm)
    slab.set_vectors(b=rhs_with_subnormals(n, 43))
    runs = []
    for parts in (15, 7, 15):
        slab.set_option("zero_start_parts", parts)
        assert slab.first_form() == 0 and slab.initial_form() == 0
        st = slab.solve(max_iters=5, tol=0.0)
        runs.append((st.iterations, st.converged, slab.history().copy()))
    assert runs[0][0] == 5 and np.isfinite(runs[0][2]).all()
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and np.array_equal(bits(r[2]), bits(runs[0][2]))
    slab.destroy()
    comm.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_the_gate_on_a_borrowed_operator(Blab, O, monkeypatch):
    """cg_solve_device around this library's stencil operator: the workspace slab borrows the matrix and takes the caller's x0, so it
    is outside the gate twice over (csrc/slab_decisions.hpp; the decision itself is tests/abi/slab_first_stage_test.cpp's, the
    workspace slab has no handle to ask). What can be seen from outside: a zero x0 solves to the same bits with SPMV_AMD_ZERO_START=0,
    the launches of before, in a workspace created anew."""
    B = Blab
    n = 640
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(O.stencil5_coo(n), n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    b = rhs_with_subnormals(n, 11)
    runs = []
    for value in (None, "0"):
        B.lib().spmv_amd_cg_release_workspace()
        if value is not None:
            monkeypatch.setenv("SPMV_AMD_ZERO_START", value)
        x, hist, st = B.cg_solve(op, m, b, np.zeros(n * n), max_iters=80, tol=1e-10, device=True)
        runs.append((st.iterations, st.converged, hist, x))
    assert runs[0][1] == 1 and same(runs[0], runs[1])
    B.lib().spmv_amd_cg_release_workspace()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
