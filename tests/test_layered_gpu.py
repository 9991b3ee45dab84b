"""The uniform-tile loop of the single-rank CG slab on anisotropic and layered stencils (tests/layered.py), against the CPU oracle and
the numpy restatements, bit for bit: stencil5_direction_block_kernel<R, true | false> with stencil5_block_list_kernel,
cg_update_r_recompute_kernel and its ap_at, stencil5_first_block_kernel, and whole solves (csrc/spmv_kernels.hip;
csrc/slab_decisions.hpp LoopShape::fused_direction, ap_recomputed, b_is_p0).

What the generator's matrix cannot show: its four off-diagonals are equal, so a fast path that hands sp.n where sp.w belongs computes
the same bits; here W = E = -1.25 and N = S = -0.75. And its only slow row blocks hold the grid's first and last grid row; here
bands of grid rows with coefficients of their own make all-slow row blocks in the interior of the grid, which keeps
LoopShape::ap_recomputed eligible: the r update reads a stored A p' beside recomputed ones, chunks straddle from a fast row block
into a slow one and back, the whole-wave fast path reads p' at +-n out of a slow neighbour block, and the launch over the slow blocks
stores A p' where the fused launch stores none. tests/test_layered_host.py holds the matrices against the table (EXPECTED)."""
import numpy as np
import pytest

import block_map as BM
import cg_restatement as CG
import layered as L
import reduction_restatement as R_
import tile_classes as T
from bitwise import bits, same_bits
from test_cg_restated_gpu import check
from test_layered_host import EXPECTED, mixed_coo
from test_zero_start_gpu import rhs, slab_of

pytestmark = pytest.mark.gpu

FUSED = "single rank: direction update inside the block SpMV"
POISON = 0xFFFFFFFFFFFFFFFF
BETA = 0.37
RR_OLD, PAP = 1.7, 3.1  # alpha = rr_old / pAp on the device
R0_ONCE = 2             # CgSlab.initial_form(): r0 stored once, x0 loaded
TOL, MAX_ITERS = 1e-8, 300
STAGE_CASES = [name for name in L.CASES if name != "bad-pick-640"]  # every case that takes LoopShape::ap_recomputed
SOLVE_CASES = ["aniso-129", "aniso-416", "layers-96", "layers-160", "layers-257", "layers-640", "misaligned-640", "r4-only-640",
               "bad-pick-640", "mixed-640"]
_cache = {}


def matrix(O, name):
    """(n, COO entries, rp, ci, va): a case of tests/layered.py, or "mixed-640" (test_layered_host.mixed_coo). Built once."""
    if name != "mixed-640":
        return L.case(O, name)
    if name not in _cache:
        n, e = mixed_coo(O)
        _cache[name] = (n, e) + tuple(O.build_csr(e, n * n))
    return _cache[name]


def layered_slab(B, O, monkeypatch, name, R):
    """The slab of a case with block_rows R. Where the slow blocks pass the product's cap (at most 1/16 of the blocks) every option
    keeps its default, so the shape is the product's own decision; elsewhere -- the small grids, and mixed-640 under R = 8, whose
    26 slow block tiles of 400 miss it by one -- fused_direction 2, the rule without the cap. bad-pick-640, nearly all slow, keeps
    the defaults too: the product's rule must turn it away."""
    n, e = matrix(O, name)[:2]
    if n < 512:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "8")
    slab = slab_of(B, e, n)
    slab.set_block_rows(R)
    passes_cap = EXPECTED[name][3][R] if name != "mixed-640" else R == 4
    if not passes_cap and name != "bad-pick-640":
        slab.set_option("fused_direction", 2)
    return slab, n


def vectors(name, n, R):
    """r, p (the fused launch's inputs) with +0.0 and -0.0 entries, by test_zero_start_gpu.rhs"""
    seed = 1000 * list(L.CASES).index(name) + R
    return rhs(n, seed), rhs(n, seed + 500)


def fast_elements(slab, n, R):
    """Element mask: its row block is fast in the whole-slab block map (every row block is all-fast or all-slow here)."""
    m = np.asarray(slab.block_map(0)).reshape(-1, T.col_tiles(n))
    assert ((m == 1).all(axis=1) | (m == 0).all(axis=1)).all()
    return np.repeat(np.repeat(m[:, 0] == 1, R)[:n], n)


def first_difference(got, want):
    d = np.flatnonzero(bits(got) != bits(want))
    return None if len(d) == 0 else (len(d), int(d[0]), float(np.asarray(got)[d[0]]), float(np.asarray(want)[d[0]]))


# ---------------------------------------------------------------- a. the class map, the block map, the slow list
@pytest.mark.parametrize("name", list(L.CASES) + ["mixed-640"])
def test_the_maps_are_the_restated_maps(Blab, O, monkeypatch, name):
    """The class map equals tile_classes.classify byte for byte and counts the table's uniform tiles; the whole-slab block map equals
    block_map.block_map, has the table's slow row blocks and no mixed one (mixed-640: exactly one, and the slab is not eligible); the
    slow list is the zero bytes of the block map."""
    n, e, rp, ci, va = matrix(O, name)
    slab, _ = layered_slab(Blab, O, monkeypatch, name, 4)
    cls, uniform, total = T.classify(rp, ci, va, n, 0, n * n)
    ct = T.col_tiles(n)
    assert np.array_equal(slab.tile_classes(), cls.reshape(-1))
    assert slab.uniform_tiles() == (uniform, total) and total == (n - 2) * ct
    if name != "mixed-640":
        assert uniform == EXPECTED[name][1]
    for R in BM.BLOCK_ROWS:
        slab.set_block_rows(R)
        m = np.asarray(slab.block_map(0)).reshape(-1, ct)
        assert np.array_equal(m, BM.block_map(cls, 0, n, R)), R
        fast, slow = (m == 1).all(axis=1), (m == 0).all(axis=1)
        mixed = int((~fast & ~slow).sum())
        want_slow, want_blocks = EXPECTED["layers-640" if name == "mixed-640" else name][2][R]
        assert (int(slow.sum()), len(m)) == (want_slow, want_blocks), R
        assert mixed == (1 if name == "mixed-640" else 0), R
        assert slab.ap_form()[2] == (mixed == 0), R
        got = slab.slow_blocks(0)
        assert got.dtype == np.int32 and np.array_equal(got, np.flatnonzero(m.reshape(-1) == 0)), R
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- b. the fused launch
def fused_launches(slab, r, p):
    """(p', A p', partials, pAp) of the fused launch with its store, and of the one without."""
    stored = slab.direction_spmv(r, p, BETA)
    slab.set_option("direction_store", 0)
    half = slab.direction_spmv(r, p, BETA)
    slab.set_option("direction_store", 1)
    return stored, half


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_the_fused_launch_is_the_oracle(Blab, O, monkeypatch, name, R):
    """direction_spmv(r, p, beta): p' = fma(1, r, beta p) by the oracle's axpby, A p' by the oracle's SpMV of p', the p.Ap partials and
    their sum by the restated reduction. The launch without the store gives the same p', partials and sum, leaves A p' alone (NaN)
    exactly on the elements of fast row blocks and holds the oracle's bits on every slow one, the interior bands included."""
    slab, n = layered_slab(Blab, O, monkeypatch, name, R)
    rp, ci, va = matrix(O, name)[2:]
    r, p = vectors(name, n, R)
    want_p = O.axpby(1.0, r, BETA, p)
    want_Ap = O.spmv_stencil5(rp, ci, va, want_p, n)
    want_partials = R_.rowlds_partials(want_p, want_Ap, n)
    want_pAp = R_.reduce(want_partials)
    fast = fast_elements(slab, n, R)
    slow_blocks, blocks = EXPECTED[name][2][R]
    assert fast.any() and int((~fast).sum()) == n * min(n, R * slow_blocks - (blocks * R - n))  # the last row block may be short
    for store, (p_new, Ap, partials, pAp) in zip((1, 0), fused_launches(slab, r, p)):
        assert first_difference(p_new, want_p) is None, (store, first_difference(p_new, want_p))
        assert len(partials) == n * T.col_tiles(n) and not (bits(partials) == POISON).any()
        assert first_difference(partials, want_partials) is None, (store, first_difference(partials, want_partials))
        assert same_bits([pAp], [want_pAp]), (store, pAp, want_pAp)
        if store:
            assert first_difference(Ap, want_Ap) is None, first_difference(Ap, want_Ap)
        else:
            assert (bits(Ap)[fast] == POISON).all()
            assert first_difference(Ap[~fast], want_Ap[~fast]) is None, first_difference(Ap[~fast], want_Ap[~fast])
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- c. the recomputing r update
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_the_recomputing_r_update_is_the_oracle(Blab, O, monkeypatch, name, R):
    """update_r_stage on p' and the A p' the launch without the store left (NaN on the fast row blocks), in both sweep directions,
    against the oracle: r = fma(-alpha, A p', r) with alpha = rr_old / pAp as the device divides, the r.r partials by the restated
    reduction of that r. Every partial slot is written; a launch that finds the solve converged writes nothing. cg_update_r_kernel on
    the oracle's A p' is held to the same reference, so a failure says which side moved."""
    slab, n = layered_slab(Blab, O, monkeypatch, name, R)
    rp, ci, va = matrix(O, name)[2:]
    assert slab.ap_form()[2]  # eligible
    r, p = vectors(name, n, R)
    want_p = O.axpby(1.0, r, BETA, p)
    want_Ap = O.spmv_stencil5(rp, ci, va, want_p, n)
    alpha = float(np.float64(RR_OLD) / np.float64(PAP))
    want_r = O.axpy(-alpha, want_Ap, r)
    want_partials = R_.residual_partials(want_r)
    assert len(want_partials) == (n * n // 2 + 63) // 64
    _, (p_new, Ap_half, _, _) = fused_launches(slab, r, p)
    assert same_bits(p_new, want_p) and np.isnan(Ap_half).any() and not np.isnan(Ap_half).all()
    for reverse in (False, True):
        plain_r, plain_partials = slab.update_r_stage(r, want_Ap, RR_OLD, PAP, reverse=reverse)
        assert first_difference(plain_r, want_r) is None, ("cg_update_r_kernel", reverse, first_difference(plain_r, want_r))
        assert first_difference(plain_partials, want_partials) is None, ("cg_update_r_kernel", reverse)
        got_r, got_partials = slab.update_r_stage(r, Ap_half, RR_OLD, PAP, p_new=p_new, reverse=reverse)
        assert len(got_partials) == len(want_partials)
        assert not (bits(got_partials) == POISON).any() and not np.isnan(got_r).any()
        assert first_difference(got_r, want_r) is None, ("recomputing", reverse, first_difference(got_r, want_r))
        assert first_difference(got_partials, want_partials) is None, ("recomputing", reverse, first_difference(got_partials, want_partials))
    got_r, got_partials = slab.update_r_stage(r, Ap_half, RR_OLD, PAP, p_new=p_new, converged=1)
    assert same_bits(got_r, r) and (bits(got_partials) == POISON).all()
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- d. the first stage
@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_the_first_stage_is_the_oracle(Blab, O, monkeypatch, name, R):
    """x0 the library's zeros, so b serves as p0: first_stage() in both sweep directions. A b by the oracle's SpMV, the b.(A b) and
    b.b partials and both sums by the restated reduction; every slot written; the stored b unchanged."""
    slab, n = layered_slab(Blab, O, monkeypatch, name, R)
    rp, ci, va = matrix(O, name)[2:]
    b = rhs(n, 31 * n + R)
    slab.set_vectors(b=b)
    assert slab.first_form() == 1
    want_Ab = O.spmv_stencil5(rp, ci, va, b, n)
    want_partials, want_bb = R_.rowlds_partials(b, want_Ab, n), R_.rowlds_partials(b, b, n)
    want_pAp, want_rr = R_.reduce(want_partials), R_.reduce(want_bb)
    for reverse in (True, False):
        Ab, partials, bb_partials, rr, pAp = slab.first_stage(reverse=reverse)
        assert len(partials) == len(bb_partials) == n * T.col_tiles(n)
        assert not (bits(partials) == POISON).any() and not (bits(bb_partials) == POISON).any()
        assert first_difference(Ab, want_Ab) is None, (reverse, first_difference(Ab, want_Ab))
        assert first_difference(partials, want_partials) is None, (reverse, first_difference(partials, want_partials))
        assert first_difference(bb_partials, want_bb) is None, (reverse, first_difference(bb_partials, want_bb))
        assert same_bits([rr, pAp], [want_rr, want_pAp]), (reverse, rr, want_rr, pAp, want_pAp)
    assert same_bits(slab.stored_b(), b)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- e. whole solves
def system(name, n):
    """b with signed zeros, and the uploaded x0"""
    return rhs(n, 3 * n + len(name)), 0.1 * np.random.default_rng(n + len(name)).standard_normal(n * n)


def restated(O, name, x0_kind):
    """The restated solve of one system: computed once, shared by both block sizes."""
    key = ("solve", name, x0_kind)
    if key not in _cache:
        n, _, rp, ci, va = matrix(O, name)
        b, x0 = system(name, n)
        _cache[key] = CG.solve(CG.whole_grid(O, rp, ci, va, n, "row-lds"), b, np.zeros(n * n) if x0_kind == "zeros" else x0, MAX_ITERS, TOL)
    return _cache[key]


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_whole_solves_are_the_restated_solve(Blab, O, monkeypatch, name, R):
    """Residual history entry by entry, iteration count, verdict and x against tests/cg_restatement.py, with x0 the library's zeros
    and x0 uploaded, ap_recompute 1 and 0 -- and the form each solve reports. The cases of the table take the fused shape and, under
    ap_recompute 1, recompute A p' in every iteration >= 1 (misaligned-640 and r4-only-640 too: a band turns every column tile of a
    row block slow, test_layered_host.py); with the library's zeros b serves as p0. mixed-640, one row block with block tiles of both
    kinds, takes the fused shape and keeps the stored A p'. bad-pick-640, whose quintuple is the band's, keeps the launches apart."""
    slab, n = layered_slab(Blab, O, monkeypatch, name, R)
    b, x0 = system(name, n)
    slab.set_vectors(b=b)
    takes = name not in ("bad-pick-640", "mixed-640")
    for x0_kind in ("zeros", "random"):
        if x0_kind == "random":
            slab.set_vectors(b=b, x0=x0)
            assert slab.first_form() == 0 and slab.initial_form() == R0_ONCE
        elif takes:
            assert slab.first_form() == 1
        want = restated(O, name, x0_kind)
        assert want[3] == 1 and want[2] > 16  # more iterations than the direction ring has slots
        for option in (1, 0):
            slab.set_option("ap_recompute", option)
            assert slab.loop_shape() == ("single rank" if name == "bad-pick-640" else FUSED)
            assert slab.ap_form()[0] == (takes and option == 1)
            st = slab.solve(max_iters=MAX_ITERS, tol=TOL)
            check((slab.gather(), slab.history(), st.iterations, st.converged), want, (name, R, x0_kind, option))
            would, took, eligible, launches = slab.ap_form()
            if takes:
                assert eligible and took == (option == 1), (x0_kind, option)
                assert (st.iterations - 1 <= launches <= st.iterations) if option == 1 else launches == 0, (option, launches, st.iterations)
            elif name == "mixed-640":
                assert (would, took, eligible, launches) == (False, False, False, 0)
            else:
                assert (would, took, launches) == (False, False, 0)
    slab.destroy()
    Blab.lib().spmv_amd_reset_host_matrices()
