"""The r update that recomputes A p' (csrc/spmv_kernels.hip cg_update_r_recompute_kernel and stencil5_direction_block_kernel<R, false>;
csrc/skew_geometry.hpp; csrc/slab_decisions.hpp LoopShape::ap_recomputed): in iterations >= 1 of the fused direction loop the fused
launch does not store A p' on its fast blocks and the r update recomputes it from p' on block tiles cut at the 128-element boundaries
of the linear index. Every result must be what the stored A p' and cg_update_r_kernel compute, bit for bit: r, every r.r partial, the
fused launch's p' and p.Ap partials, whole solves. Grids: 12 (one chunk spans more than ten grid rows), 96 (no chunk lies inside a grid row), 127 /
129 / 255 / 257 (odd: unaligned +-n pairs, an odd n^2 whose last element rides in chunk 0), 128 (no skew), 160, 416 (416 = 32 mod 128,
the skew of the 20 000 grid)."""
import numpy as np
import pytest

import tile_classes as T
from bitwise import bits, same_bits
from test_zero_start_gpu import rhs, slab_of

GRIDS = [12, 96, 127, 128, 129, 160, 255, 257, 416]
POISON = 0xFFFFFFFFFFFFFFFF
RR_OLD, PAP = 1.7, 3.1  # alpha = rr_old / pAp on the device


def fused_option(n, R):
    """The product's rule (slow blocks at most 1/16 of the blocks) where the grid is large enough for it, else the rule without the cap."""
    blocks = -(-n // R)
    return 1 if 16 * 2 <= blocks else 2


def generator_slab(B, O, monkeypatch, n, R):
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "8")
    slab = slab_of(B, O.stencil5_coo(n), n)
    slab.set_block_rows(R)
    slab.set_option("fused_direction", fused_option(n, R))
    return slab


def fast_elements(slab, n, R):
    """Element mask: its row block is fast in the whole-slab block map (every row block is all-fast or all-slow here)."""
    m = np.asarray(slab.block_map(0)).reshape(-1, T.col_tiles(n))
    assert ((m == 1).all(axis=1) | (m == 0).all(axis=1)).all()
    return np.repeat(np.repeat(m[:, 0] == 1, R)[:n], n)


def one_solve(slab, **solve):
    st = slab.solve(**solve)
    return st.iterations, st.converged, slab.history().copy(), slab.gather()


def same(a, b):
    return a[:2] == b[:2] and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", GRIDS)
def test_both_launches_alone_equal_the_stored_form_bit_for_bit(Blab, O, monkeypatch, n, R):
    """The fused launch with and without the store: p' and every p.Ap partial and their sum equal; A p' is left alone (NaN) exactly on
    the fast row blocks and stored on the slow ones. Then the r update given p' and that half-filled A p' against cg_update_r_kernel
    given the stored A p', in both sweep directions: r and every partial equal, every partial slot written. A launch that finds the solve
    converged only reads."""
    slab = generator_slab(Blab, O, monkeypatch, n, R)
    assert slab.ap_form()[2]  # eligible
    rng = np.random.default_rng(100 * n + R)
    r, p = rhs(n, 7 * n + R), rng.standard_normal(n * n)
    p_new, Ap, partials, pAp = slab.direction_spmv(r, p, 0.37)
    assert not np.isnan(Ap).any()
    slab.set_option("direction_store", 0)
    p_new2, Ap2, partials2, pAp2 = slab.direction_spmv(r, p, 0.37)
    slab.set_option("direction_store", 1)
    assert same_bits(p_new2, p_new) and same_bits(partials2, partials) and same_bits([pAp2], [pAp])
    fast = fast_elements(slab, n, R)
    assert (bits(Ap2)[fast] == POISON).all() and same_bits(Ap2[~fast], Ap[~fast])
    if (n, R) != (12, 8):  # (two row blocks there: one holds the grid's first grid row, the other is short)
        assert fast.any()
    count = (n * n // 2 + 63) // 64
    for reverse in (False, True):
        want_r, want_partials = slab.update_r_stage(r, Ap, RR_OLD, PAP, reverse=reverse)
        got_r, got_partials = slab.update_r_stage(r, Ap2, RR_OLD, PAP, p_new=p_new, reverse=reverse)
        assert len(want_partials) == len(got_partials) == count
        assert not (bits(got_partials) == POISON).any() and not np.isnan(got_r).any()
        assert same_bits(got_r, want_r), (reverse, int((bits(got_r) != bits(want_r)).sum()))
        assert same_bits(got_partials, want_partials), reverse
    got_r, got_partials = slab.update_r_stage(r, Ap2, RR_OLD, PAP, p_new=p_new, converged=1)
    assert same_bits(got_r, r) and (bits(got_partials) == POISON).all()
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("n", GRIDS)
def test_whole_solves_are_bit_identical_with_a_p_recomputed(Blab, O, monkeypatch, n, R):
    """Option 1 against option 0, alternated, random b: to convergence (run_ahead 2: one iteration is enqueued past convergence, whose
    launches must return on the scalars) and five iterations at tolerance 0. x, residual history, iterations and verdict equal; under
    option 1 the form WAS taken, with one recomputing launch per iteration >= 1; under option 0 it was not."""
    slab = generator_slab(Blab, O, monkeypatch, n, R)
    slab.set_vectors(b=rhs(n, 3 * n + R))
    for solve, run_ahead in (({"max_iters": 200, "tol": 1e-10}, 2), ({"max_iters": 5, "tol": 0.0}, 1)):
        slab.set_option("run_ahead", run_ahead)
        runs = []
        for option in (0, 1, 0, 1, 1):
            slab.set_option("ap_recompute", option)
            assert slab.ap_form()[0] == (option == 1)
            runs.append(one_solve(slab, **solve))
            would, took, eligible, launches = slab.ap_form()
            assert eligible and took == (option == 1), (option, solve)
            iterations = runs[-1][0]
            assert (iterations - 1 <= launches <= iterations) if option == 1 else launches == 0, (option, launches, iterations)
        assert runs[0][0] > 1 and (runs[0][1] == 1 or solve["tol"] == 0.0)
        for k, run in enumerate(runs[1:]):
            assert same(run, runs[0]), (k + 1, solve)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [81, 512])
def test_the_golden_history_with_a_p_recomputed(Blab, O, golden, monkeypatch, n):
    """The generator's system (b = 1, x0 = 0) on grids 81 and 512 against tests/golden/known_answers.json, with the form taken; and
    option 0 gives the same bits."""
    monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "8")
    Blab.lib().spmv_amd_reset_host_matrices()
    slab = Blab.CgSlab.stencil5(n)
    slab.set_option("fused_direction", fused_option(n, 4))
    gold = golden["cases"][f"{n}:5.0"]["cg"]
    got = one_solve(slab)
    assert slab.ap_form()[1] and slab.ap_form()[3] >= got[0] - 1
    want = np.array(gold["history"])
    assert got[0] == gold["iterations"] and got[1] == gold["converged"] and len(got[2]) == len(want)
    assert np.max(np.abs(got[2] - want) / want) < 1e-10
    slab.set_option("ap_recompute", 0)
    assert same(one_solve(slab), got) and not slab.ap_form()[1]
    slab.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 8])
def test_a_row_block_that_is_neither_fast_nor_slow_keeps_the_stored_form(Blab, O, R):
    """One perturbed centre in grid row 70 of n = 640: one block tile of a row block that is fast otherwise goes through the slow list,
    so that row block is mixed. The slab reports the form NOT taken under option 1, refuses the recomputing launch, and solves to
    option 0's bits."""
    n = 640
    e = O.stencil5_coo(n)
    T.set_entry(e, 70 * n + 129, 70 * n + 129, np.nextafter(5.0, 6.0))
    slab = slab_of(Blab, e, n)
    slab.set_block_rows(R)
    m = np.asarray(slab.block_map(0)).reshape(-1, T.col_tiles(n))
    assert m[70 // R].sum() == T.col_tiles(n) - 1  # mixed
    slab.set_vectors(b=rhs(n, 5))
    assert slab.loop_shape() == "single rank: direction update inside the block SpMV"
    assert slab.ap_form()[:3] == (False, False, False)
    with pytest.raises(RuntimeError):
        slab.update_r_stage(np.zeros(n * n), np.zeros(n * n), RR_OLD, PAP, p_new=np.zeros(n * n))
    got = one_solve(slab, max_iters=80, tol=1e-10)
    assert slab.ap_form() == (False, False, False, 0) and got[1] == 1
    slab.set_option("ap_recompute", 0)
    assert same(one_solve(slab, max_iters=80, tol=1e-10), got)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_a_borrowed_operator_keeps_the_stored_form(Blab, O, monkeypatch):
    """cg_solve_device around this library's stencil operator: the workspace slab borrows the matrix, reports the form not taken, and
    solves to the same bits with SPMV_AMD_AP_RECOMPUTE=0 in a workspace created anew."""
    B = Blab
    n = 640
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(O.stencil5_coo(n), n * n, n * n, n)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    b = rhs(n, 11)
    runs = []
    for value in (None, "0"):
        B.lib().spmv_amd_cg_release_workspace()
        if value is not None:
            monkeypatch.setenv("SPMV_AMD_AP_RECOMPUTE", value)
        x, hist, st = B.cg_solve(op, m, b, np.zeros(n * n), max_iters=80, tol=1e-10, device=True)
        runs.append((st.iterations, st.converged, hist, x))
        form = B.CgSlab.workspace_ap_form()
        assert form is not None and form[:2] == (False, False) and form[3] == 0
    assert runs[0][1] == 1 and same(runs[0], runs[1])
    B.lib().spmv_amd_cg_release_workspace()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()
