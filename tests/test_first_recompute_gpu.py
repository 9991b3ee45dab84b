"""Iteration 0 in the store-less form (csrc/slab_decisions.hpp LoopShape::first_recomputed, first_form; csrc/spmv_kernels.hip
stencil5_first_block_kernel<R, false>, stencil5_rowlds_block_kernel<R, false> and cg_update_r_recompute_kernel<R, true>): where the
loop recomputes A p' in its r updates, iteration 0's SpMV does not store A p0 on its fast blocks either and its r update recomputes
it from the ONE vector that is both r0 and p0 -- b on a zero start, ring slot 0 on a caller's x0. Every result must be what the stored
A p0 and cg_update_r_from_kernel compute, bit for bit: both partial arrays and both sums of the first launch, r and every r.r partial,
whole solves. Grids as in test_ap_recompute_gpu.py (12: a chunk spans more than ten grid rows; 96: no chunk inside a grid row; 127 /
129 / 255 / 257: odd, the whole-wave path starts at 257; 128: no skew; 160; 416: the skew of the 20 000 grid) and 640 (five column
tiles)."""
import numpy as np
import pytest

import test_layered_gpu as TL
import tile_classes as T
from bitwise import bits, same_bits
from test_ap_recompute_gpu import fast_elements, fused_option, generator_slab, one_solve, same
from test_first_stage_gpu import rhs_with_subnormals
from test_zero_start_gpu import rhs

GRIDS = [12, 96, 127, 128, 129, 160, 255, 257, 416, 640]
POISON = 0xFFFFFFFFFFFFFFFF
RR_OLD, PAP = 1.7, 3.1  # alpha = rr_old / pAp on the device
STORED, FROM_B, FROM_SLOT0, IN_PLACE = "stored", "from b", "from ring slot 0", "in place"


def r_update_both_ways(slab, src, Ap_stored, Ap_half, n):
    """The out-of-place recomputing instance on (src, the half-filled A src) against cg_update_r_from_kernel on (the stored A src, src),
    both sweep directions: r and every partial equal, every slot written, src untouched; a converged solve writes nothing."""
    count = (n * n // 2 + 63) // 64
    for reverse in (False, True):
        want_r, want_src, want_partials = slab.update_r_from_stage(src, Ap_stored, RR_OLD, PAP, recompute=False, reverse=reverse)
        got_r, got_src, got_partials = slab.update_r_from_stage(src, Ap_half, RR_OLD, PAP, recompute=True, reverse=reverse)
        assert len(want_partials) == len(got_partials) == count
        assert not (bits(got_partials) == POISON).any() and not (bits(got_r) == POISON).any()
        assert same_bits(got_r, want_r), (reverse, int((bits(got_r) != bits(want_r)).sum()))
        assert same_bits(got_partials, want_partials), reverse
        assert same_bits(got_src, src) and same_bits(want_src, src)
    got_r, got_src, got_partials = slab.update_r_from_stage(src, Ap_half, RR_OLD, PAP, recompute=True, converged=1)
    assert (bits(got_r) == POISON).all() and (bits(got_partials) == POISON).all() and same_bits(got_src, src)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", GRIDS)
def test_both_launches_of_iteration_0_alone_equal_the_stored_form(Blab, O, monkeypatch, n, R):
    """b random with signed zeros and subnormals. The first launch on b with its store switched off against on, both sweep directions:
    both partial arrays and both sums equal, A b left alone (NaN) exactly on the fast row blocks and equal on the slow ones. Then the
    r update from b. Then the same through the block kernel on an uploaded p0 (r0 in ring slot 0), and the r update from that p0."""
    slab = generator_slab(Blab, O, monkeypatch, n, R)
    both_launches_alone(slab, n, R, allow_no_fast=(n, R) == (12, 8))  # (two row blocks there: one holds the grid's first grid row, the other is short)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", ["aniso-129", "aniso-257", "aniso-416", "layers-160", "layers-257", "layers-640"])
def test_both_launches_of_iteration_0_alone_on_anisotropic_and_layered_stencils(Blab, O, monkeypatch, name, R):
    """The same on tests/layered.py's matrices: W = E differ from N = S, so a chain that hands one where the other belongs computes
    other bits, and the layered cases have all-slow row blocks inside the grid, where the r update reads the stored A p0 beside
    recomputed ones and the whole-wave path (n >= 257) reads p0 at +-n out of a slow neighbour block."""
    slab, n = TL.layered_slab(Blab, O, monkeypatch, name, R)
    both_launches_alone(slab, n, R)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


def both_launches_alone(slab, n, R, allow_no_fast=False):
    assert slab.ap_form()[2]  # eligible
    b = rhs_with_subnormals(n, 13 * n + R)
    b[n * n // 2] = -0.0
    slab.set_vectors(b=b)
    assert slab.first_form() == 1 and slab.first_recompute_form()[0] == FROM_B
    fast = fast_elements(slab, n, R)
    assert fast.any() or allow_no_fast
    for reverse in (True, False):
        Ab, partials, bb_partials, rr, pAp = slab.first_stage(reverse=reverse)
        slab.set_option("first_store", 0)
        Ab2, partials2, bb_partials2, rr2, pAp2 = slab.first_stage(reverse=reverse)
        slab.set_option("first_store", 1)
        assert not (bits(Ab) == POISON).any()
        assert not (bits(partials2) == POISON).any() and not (bits(bb_partials2) == POISON).any()
        assert same_bits(partials2, partials) and same_bits(bb_partials2, bb_partials) and same_bits([rr2, pAp2], [rr, pAp]), reverse
        assert (bits(Ab2)[fast] == POISON).all() and same_bits(Ab2[~fast], Ab[~fast]), reverse
    assert same_bits(slab.stored_b(), b)
    r_update_both_ways(slab, b, Ab, Ab2, n)
    # the block kernel, as iteration 0 on a caller's x0 runs it on p0 = r0 in ring slot 0
    p0 = rhs(n, 17 * n + R)
    slab.set_option("spmv_with_dot", 1)
    Ap = slab.spmv(p0)
    partials, pAp = slab.spmv_dot()
    slab.set_option("first_store", 0)
    Ap2 = slab.spmv(p0)
    partials2, pAp2 = slab.spmv_dot()
    slab.set_option("first_store", 1)
    slab.set_option("spmv_with_dot", 0)
    assert not np.isnan(Ap).any() and not (bits(partials2) == POISON).any()
    assert same_bits(partials2, partials) and same_bits([pAp2], [pAp])
    assert (bits(Ap2)[fast] == POISON).all() and same_bits(Ap2[~fast], Ap[~fast])
    r_update_both_ways(slab, p0, Ap, Ap2, n)


SOLVES = [({"max_iters": 200, "tol": 1e-10}, 2), ({"max_iters": 200, "tol": 1e-10}, 0), ({"max_iters": 0, "tol": 0.0}, 1),
          ({"max_iters": 1, "tol": 0.0}, 2), ({"max_iters": 5, "tol": 0.0}, 0), ({"max_iters": 200, "tol": 0.9}, 2)]


def solves_each_way(slab, want_form, solves=SOLVES):
    """first_recompute 0, 1, 0, 1, 1 on one slab for each (solve, run_ahead): x, history, iterations and verdict equal; the accessor
    says which form iteration 0 took; ap_form()'s count stays the launches of iterations >= 1."""
    for solve, run_ahead in solves:
        slab.set_option("run_ahead", run_ahead)
        runs = []
        for option in (0, 1, 0, 1, 1):
            slab.set_option("first_recompute", option)
            expect = want_form if option == 1 else STORED
            assert slab.first_recompute_form()[0] == expect
            runs.append(one_solve(slab, **solve))
            assert slab.first_recompute_form() == (expect, expect if solve["max_iters"] > 0 else STORED), (option, solve)
            would, took, eligible, launches = slab.ap_form()
            iterations = runs[-1][0]
            assert eligible and took, (option, solve)
            assert iterations - 1 <= launches <= iterations if iterations > 0 else launches == 0, (option, launches, iterations)
        if solve["tol"] == 0.9:
            assert runs[0][:2] == (1, 1)  # converged in iteration 0
        for k, run in enumerate(runs[1:]):
            assert same(run, runs[0]), (k + 1, solve, run_ahead)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", [416, 1003])
def test_whole_solves_are_bit_identical_with_iteration_0_recomputed(Blab, O, monkeypatch, n, R):
    """Zero start (b serves as p0) and an uploaded x0 (r0 in ring slot 0); to convergence, 0 / 1 / 5 iterations at tolerance 0,
    convergence in iteration 0; run_ahead 0 and 2 (one iteration enqueued past convergence); a timeline solve."""
    slab = generator_slab(Blab, O, monkeypatch, n, R)
    b = rhs(n, 3 * n + R)
    slab.set_vectors(b=b)
    solves_each_way(slab, FROM_B)
    for option in (0, 1):  # with the stage marks of a timeline solve
        slab.set_option("first_recompute", option)
        st, _ = slab.timeline_solve(max_iters=200, tol=1e-10)
        run = (st.iterations, st.converged, slab.history().copy(), slab.gather())
        first = run if option == 0 else first
        assert same(run, first) and slab.first_recompute_form()[1] == (FROM_B if option else STORED)
    assert same_bits(slab.stored_b(), b)
    slab.set_vectors(b=b, x0=0.1 * np.random.default_rng(n + R).standard_normal(n * n))
    assert slab.first_form() == 0
    solves_each_way(slab, FROM_SLOT0)
    # r0 stored twice (zero_start off): the in-loop in-place instance takes iteration 0 too
    slab.set_option("zero_start", 0)
    solves_each_way(slab, IN_PLACE, SOLVES[:1] + SOLVES[3:5])
    assert same_bits(slab.stored_b(), b)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["2", "4", "16"])
def test_b_stands_for_ring_slot_0_across_a_wrap(Blab, O, monkeypatch, ring):
    """Rings 2, 4 and 16 on n = 416 (the solve is longer than each): the first window's flush reads b as slot 0, the real slot 0 is
    written when the ring wraps."""
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    n, R = 416, 8
    slab = generator_slab(Blab, O, monkeypatch, n, R)
    b = rhs(n, 5 * n + int(ring))
    slab.set_vectors(b=b)
    solves_each_way(slab, FROM_B, SOLVES[:2] + SOLVES[4:5])
    slab.set_vectors(b=b, x0=0.1 * np.random.default_rng(int(ring)).standard_normal(n * n))
    solves_each_way(slab, FROM_SLOT0, SOLVES[:1])
    assert same_bits(slab.stored_b(), b)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
def test_a_layered_matrix_takes_the_form_and_is_the_restated_solve(Blab, O, monkeypatch, R):
    """layers-257 (tests/layered.py): all-slow row blocks inside the grid, W = E and N = S different -- iteration 0's r update reads a
    stored A p0 beside recomputed ones. Zero start and uploaded x0 against tests/cg_restatement.py, with the form taken."""
    name = "layers-257"
    slab, n = TL.layered_slab(Blab, O, monkeypatch, name, R)
    fast = fast_elements(slab, n, R)
    rows_fast = fast.reshape(n, n)[:, 0]
    assert (~rows_fast[R:-R]).any() and rows_fast.any()  # slow row blocks other than the first and the last
    b, x0 = TL.system(name, n)
    slab.set_vectors(b=b)
    for x0_kind, form in (("zeros", FROM_B), ("random", FROM_SLOT0)):
        if x0_kind == "random":
            slab.set_vectors(b=b, x0=x0)
        want = TL.restated(O, name, x0_kind)
        for option in (1, 0):
            slab.set_option("first_recompute", option)
            st = slab.solve(max_iters=TL.MAX_ITERS, tol=TL.TOL)
            TL.check((slab.gather(), slab.history(), st.iterations, st.converged), want, (name, R, x0_kind, option))
            assert slab.first_recompute_form()[1] == (form if option == 1 else STORED)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
def test_a_mixed_row_block_keeps_the_stored_form(Blab, O, monkeypatch, R):
    """mixed-640: one row block with block tiles of both kinds. The slab is not eligible, reports the form not taken under option 1
    and solves to option 0's bits."""
    name = "mixed-640"
    slab, n = TL.layered_slab(Blab, O, monkeypatch, name, R)
    b, _ = TL.system(name, n)
    slab.set_vectors(b=b)
    runs = []
    for option in (1, 0):
        slab.set_option("first_recompute", option)
        assert slab.first_recompute_form()[0] == STORED and not slab.ap_form()[2]
        runs.append(one_solve(slab, max_iters=TL.MAX_ITERS, tol=TL.TOL))
        assert slab.first_recompute_form()[1] == STORED and slab.ap_form()[3] == 0
    assert runs[0][1] == 1 and same(runs[0], runs[1])
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [81, 512])
def test_the_golden_history_with_iteration_0_recomputed(Blab, O, golden, monkeypatch, n):
    """The generator's system (b = 1, x0 = 0) on grids 81 and 512 against tests/golden/known_answers.json with every default (8-row
    blocks, the form taken from b); option 0 gives the same bits."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "8")
    Blab.lib().spmv_amd_reset_host_matrices()
    slab = Blab.CgSlab.stencil5(n)
    slab.set_option("fused_direction", fused_option(n, 8))
    gold = golden["cases"][f"{n}:5.0"]["cg"]
    got = one_solve(slab)
    assert slab.first_recompute_form() == (FROM_B, FROM_B) and slab.ap_form()[1]
    want = np.array(gold["history"])
    assert got[0] == gold["iterations"] and got[1] == gold["converged"] and len(got[2]) == len(want)
    assert np.max(np.abs(got[2] - want) / want) < 1e-10
    slab.set_option("first_recompute", 0)
    assert same(one_solve(slab), got) and slab.first_recompute_form()[1] == STORED
    slab.destroy()


@pytest.mark.gpu
def test_eight_row_blocks_are_the_default_where_the_fused_loop_runs(Blab, O, monkeypatch):
    """A single-rank slab that owns its matrix gets 8-row block tiles by default (csrc/slab_decisions.hpp default_block_rows), 4 with
    the in-place form or with SPMV_AMD_ROWLDS_BLOCK_ROWS=4; the solves agree bit for bit."""
    n = 640
    ct = T.col_tiles(n)
    runs = []
    for env, rows in (({}, 8), ({"SPMV_AMD_ROWLDS_BLOCK_ROWS": "4"}, 4), ({"SPMV_AMD_P_RING": "1"}, 4), ({"SPMV_AMD_FUSED_DIRECTION": "0"}, 4)):
        for name in ("SPMV_AMD_ROWLDS_BLOCK_ROWS", "SPMV_AMD_P_RING", "SPMV_AMD_FUSED_DIRECTION"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        Blab.lib().spmv_amd_reset_host_matrices()
        slab = Blab.CgSlab.stencil5(n)
        assert len(slab.block_map(0)) == -(-n // rows) * ct, (env, rows)
        runs.append(one_solve(slab, max_iters=80, tol=1e-10))
        slab.destroy()
    assert runs[0][1] == 1 and all(same(run, runs[0]) for run in runs[1:])

