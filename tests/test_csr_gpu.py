"""The general CSR operator held to tests/csr_restatement.py bit for bit: the row sums of every variant on the adaptive table (one
scenario of the chunk walk per block), with finite and with poisoned x; the fused p.Ap partials of the stream and adaptive kernels,
read through the LAB build's spmv_amd_operator_fused_spmv, on matrices whose long rows are owned by threads of every wave; the same
hook on the ELLPACK operator; and whole cg_solve_device solves under each forced variant. Caller-owned vectors sit between sentinels,
at a 16-byte aligned address and 8 bytes off it; outputs start as NaN, inputs keep their bits. No tolerance anywhere."""
import functools

import numpy as np
import pytest

import cg_restatement as CG
import csr_restatement as CR
import matrices as M
import poison as P
import reduction_restatement as R
from bitwise import same_bits, same_bits_nan_as_class
from test_cg_restated_gpu import check
from test_chebyshev_gpu import Guarded
from test_mg_multi_stages_gpu import Shifted

pytestmark = pytest.mark.gpu

FORCED = [None, "stream", "adaptive", "row-scalar", "wavefront"]


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def hold(B, values, shift):
    return Shifted(B, values, 1) if shift else Guarded(B, values)


@functools.lru_cache(maxsize=None)
def table_sums(variant, poisoned):
    """The restated row sums of the table under a variant word: computed once, shared, never written."""
    t = CR.adaptive_table()
    with np.errstate(invalid="ignore"):
        y = CR.row_sums(t.rp, t.ci, t.va, t.x_poisoned if poisoned else t.x, variant)
    y.setflags(write=False)
    return y


# ---------------------------------------------------------------- the table, through every variant
@pytest.mark.parametrize("forced", FORCED)
def test_the_table_through_every_variant(B, O, forced):
    t = CR.adaptive_table()
    word = CR.variant_of(t.rp, None if forced is None else "csr/" + forced)
    op = B.Operator("cusparse-csr")
    op.select_variant(forced)
    try:
        assert op.init(B.HostMatrix(CR.entries_of(t.rp, t.ci, t.va), 145, CR.TABLE_COLS, -1)) == 0
        assert op.variant() == "csr/" + word and (forced is not None or word == "adaptive")
        want, want_p = table_sums(word, False), table_sums(word, True)
        if word in ("stream", "row-scalar"):
            assert same_bits(want, O.spmv_csr(t.rp, t.ci, t.va, t.x))
        finite = np.isfinite(want_p)
        assert np.flatnonzero(~finite).tolist() == P.poisoned_rows(t.rp, t.ci, t.reserved, []).tolist()
        got, _ = op.run_timed(t.x)
        assert same_bits(got, want), (forced, np.flatnonzero(got != want)[:8])
        got_p, _ = op.run_timed(t.x_poisoned)
        assert same_bits_nan_as_class(got_p, want_p), forced
        assert same_bits(got_p[finite], got[finite]), forced
        for shift in (0, 1):
            for x, ref, exact in ((t.x, want, True), (t.x_poisoned, want_p, False)):
                dx, dy = hold(B, x, shift), hold(B, np.full(145, np.nan), shift)
                try:
                    assert op.run_device(dx, dy) == 0
                    y = dy.read()
                    assert same_bits(y, ref) if exact else same_bits_nan_as_class(y, ref), (forced, shift, exact)
                    assert same_bits(y[finite], want[finite]), (forced, shift)
                    assert same_bits(dx.read(), x), (forced, shift)
                finally:
                    dx.free(), dy.free()
    finally:
        op.free()
        op.select_variant(None)


@pytest.mark.parametrize("forced", FORCED[1:])
def test_sums_worked_out_by_hand(B, forced):
    """csr_restatement.hand_made: expected values from integer arithmetic around 2^53, not from any code."""
    rp, ci, va, cols, want = CR.hand_made()
    op = B.Operator("cusparse-csr")
    op.select_variant(forced)
    try:
        assert op.init(B.HostMatrix(CR.entries_of(rp, ci, va), 17, cols, -1)) == 0 and op.variant() == "csr/" + forced
        got, _ = op.run_timed(np.ones(cols))
        for row, value in want[forced].items():
            assert same_bits(got[row], value), (forced, row, got[row] - 2.0 ** 53)
        assert same_bits(got[0], 0.0) and same_bits(got[2:16], np.full(14, 3.0))
    finally:
        op.free()
        op.select_variant(None)


# ---------------------------------------------------------------- the fused partials
def fused_matrix(name):
    if name == "table-square":
        rp, ci, va = CR.table_square()
        return rp, ci, va, len(rp) - 1
    a = CR.arrow(int(name.split("-")[1]))
    return a.rp, a.ci, a.va, a.n


@pytest.mark.parametrize("name", ["table-square", "arrow-3000", "arrow-8192"])
def test_fused_partials_of_the_stream_and_adaptive_kernels(Blab, O, name):
    """y and one partial per logical block from ONE fused launch, as cg_solve_device's loop makes it. per_block comes from the
    restatement of csr_stream_geometry and is confirmed by the launch's own count."""
    rp, ci, va, n = fused_matrix(name)
    per_block, blocks = CR.stream_geometry(n, len(ci))
    x = np.random.default_rng(len(ci)).standard_normal(n)
    Blab.lib().spmv_amd_reset_host_matrices()
    op = Blab.Operator("cusparse-csr")
    try:
        assert op.init(Blab.HostMatrix(CR.entries_of(rp, ci, va), n, n, -1)) == 0 and op.variant() == "csr/adaptive"
        for variant in CR.VARIANTS:
            assert op.select_variant(variant) == 0 and op.variant() == "csr/" + variant
            if variant in ("row-scalar", "wavefront"):  # no fused form: refused, nothing written
                dx, dy, dp = Guarded(Blab, x), Guarded(Blab, np.full(n, np.nan)), Guarded(Blab, np.full(blocks, np.nan))
                try:
                    rc, count = Blab.fused_spmv(op, dx, dy, dp, blocks)
                    assert rc != 0 and count == -1 and np.all(np.isnan(dy.read())) and np.all(np.isnan(dp.read())), variant
                finally:
                    dx.free(), dy.free(), dp.free()
                continue
            y = CR.row_sums(rp, ci, va, x, variant)
            want = CR.stream_block_partials(x, y, per_block)
            assert len(want) == blocks
            for shift in (0, 1):
                dx, dy, dp = hold(Blab, x, shift), hold(Blab, np.full(n, np.nan), shift), hold(Blab, np.full(blocks, np.nan), shift)
                try:
                    rc, count = Blab.fused_spmv(op, dx, dy, dp, blocks - 1)  # cap below the partial count: refused, nothing written
                    assert rc != 0 and count == -1 and np.all(np.isnan(dp.read())) and np.all(np.isnan(dy.read()))
                    rc, count = Blab.fused_spmv(op, dx, dy, dp, blocks)
                    assert rc == 0 and count == blocks, (name, variant, rc, count, blocks)
                    assert same_bits(dy.read(), y), (name, variant, shift)
                    got = dp.read()
                    assert same_bits(got, want), (name, variant, shift, np.flatnonzero(got != want)[:8])
                    assert same_bits(dx.read(), x)
                finally:
                    dx.free(), dy.free(), dp.free()
    finally:
        op.free()
        op.select_variant(None)
        Blab.lib().spmv_amd_reset_host_matrices()


def test_the_rectangular_table_has_no_fused_form(Blab):
    """The table itself is 145 x 6000: the fused partials index x by the row and exist on square operators only, so the hook refuses
    it under every variant (its partial geometry, per_block 16, is that of table-square above)."""
    t = CR.adaptive_table()
    Blab.lib().spmv_amd_reset_host_matrices()
    op = Blab.Operator("cusparse-csr")
    dx, dy, dp = Guarded(Blab, t.x), Guarded(Blab, np.full(145, np.nan)), Guarded(Blab, np.full(10, np.nan))
    try:
        assert op.init(Blab.HostMatrix(CR.entries_of(t.rp, t.ci, t.va), 145, CR.TABLE_COLS, -1)) == 0
        for forced in FORCED:
            assert op.select_variant(forced) == 0
            rc, count = Blab.fused_spmv(op, dx, dy, dp, 10)
            assert rc != 0 and count == -1 and np.all(np.isnan(dy.read())) and np.all(np.isnan(dp.read())), forced
    finally:
        dx.free(), dy.free(), dp.free()
        op.free()
        op.select_variant(None)
        Blab.lib().spmv_amd_reset_host_matrices()


def ell_case(O, rows):
    if rows == 130 * 130:
        e = O.stencil5_coo(130)
        e["value"] = np.random.default_rng(130).uniform(-3.0, 3.0, len(e))
        return e, 130
    e, _, _ = M.random_sparse(rows, rows, lambda row, rng: 0 if row % 13 == 5 else int(rng.integers(1, 8)), seed=rows)
    return e, -1


@pytest.mark.parametrize("rows", [255, 256, 257, 130 * 130])
def test_fused_partials_of_the_ellpack_operator(Blab, O, rows):
    """ell_block_dot through the same hook: until now only a whole solve reached these partials."""
    e, grid = ell_case(O, rows)
    rp, ci, va = O.build_csr(e, rows)
    x = np.random.default_rng(rows + 1).standard_normal(rows)
    y = O.spmv_csr(rp, ci, va, x)
    want = R.ell_partials(x, y)
    blocks = (rows + 255) // 256
    assert len(want) == blocks
    Blab.lib().spmv_amd_reset_host_matrices()
    op = Blab.Operator("ellpack")
    try:
        assert op.init(Blab.HostMatrix(e, rows, rows, grid)) == 0 and op.variant() == "ell/slot-major"
        for shift in (0, 1):
            dx, dy, dp = hold(Blab, x, shift), hold(Blab, np.full(rows, np.nan), shift), hold(Blab, np.full(blocks, np.nan), shift)
            try:
                rc, count = Blab.fused_spmv(op, dx, dy, dp, blocks)
                assert rc == 0 and count == blocks
                assert same_bits(dy.read(), y) and same_bits(dp.read(), want) and same_bits(dx.read(), x), (rows, shift)
            finally:
                dx.free(), dy.free(), dp.free()
    finally:
        op.free()
        Blab.lib().spmv_amd_reset_host_matrices()


# ---------------------------------------------------------------- whole solves
@pytest.mark.parametrize("variant", CR.VARIANTS)
def test_cg_solve_device_on_the_csr_operator_is_the_restated_solve(B, O, variant):
    """8 iterations from a non-zero x0 under tolerance 0 on the N = 3000 arrow matrix: x, every entry of the history, the iteration
    count and the verdict. stream / adaptive take the fused partials, row-scalar / wavefront the unfused loop."""
    a = CR.arrow(3000)
    rng = np.random.default_rng(3000)
    b, x0 = rng.standard_normal(a.n), 0.1 * rng.standard_normal(a.n)
    want = CG.solve(CR.system(O, a.rp, a.ci, a.va, variant), b, x0, 8, 0.0)
    assert want[2:] == (8, 0)
    m = B.HostMatrix(CR.entries_of(a.rp, a.ci, a.va), a.n, a.n, -1)
    op = B.Operator("cusparse-csr")
    op.select_variant(variant)
    try:
        assert op.init(m) == 0 and op.variant() == "csr/" + variant
        B.lib().spmv_amd_cg_release_workspace()
        x, hist, st = B.cg_solve(op, m, b, x0, max_iters=8, tol=0.0, device=True)
        check((x, hist, st.iterations, st.converged), want, variant)
    finally:
        op.free()
        op.select_variant(None)
