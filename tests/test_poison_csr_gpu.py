"""Poisoned inputs on the GPU, general CSR: the AMG transfers (csrc/amg.hip, csrc/amg_multi.hip), the block product and the fused p.Ap
partials of the CSR operator, and the AMG set-up on a CSR as a file gives it. Every system comes from the "general CSR" section of
tests/poison.py, where tests/test_poison_csr_host.py holds it: the reference's non-finite coarse rows are exactly the planted set,
most rows stay finite, and wrong models of the transfers that the finite stage tests cannot see are caught by these cases. Here the
kernels run on them: the result matches the reference through same_bits_nan_as_class, and every value whose inputs are the clean
level's has the bits of the clean run -- a leak between the members of a round, between rounds, between the eight groups of a wave,
between waves or between the columns of a block shows as a non-finite value the reference does not have, a sum or a chain started at
the wrong place as a zero of the wrong sign. Outputs start as NaN, inputs keep their bits, paddings keep theirs. No whole solve runs
on poisoned data. No tolerance anywhere."""
import functools

import numpy as np
import pytest

import amg_restatement as AMG
import csr_restatement as CR
import gcr_restatement as GR
import pcg_multi_amg_restatement as PA
import poison as P
from bitwise import same_bits, same_bits_nan_as_class
from test_amg_stages_gpu import Padded
from test_chebyshev_gpu import Guarded
from test_mg_multi_stages_gpu import Shifted, column, interleaved

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 8)


@pytest.fixture(autouse=True)
def _gpu(B, Blab):
    Blab.require_gpu()
    for lib in (B.lib(), Blab.lib()):
        lib.spmv_amd_set_device(0)
        lib.spmv_amd_reset_host_matrices()
    yield
    for lib in (B.lib(), Blab.lib()):
        lib.spmv_amd_reset_host_matrices()


def holder(B, shift):
    """Block vectors at a 16-byte aligned address, or 8 bytes past one."""
    return (lambda v: Shifted(B, v, shift)) if shift else (lambda v: Guarded(B, v))


def shifts_of(k):
    return (0, 1) if k % 2 == 1 else (0,)


# ---------------------------------------------------------------- restriction, single vector
def run_restrict(Blab, L, rp, ci, va, z, r, fixed):
    """One launch of the stage on a case's arrays; `fixed`: the uploaded agg_ptr and members. Returns r_c; asserts that the seven
    inputs keep their bits (the holders assert the paddings)."""
    arrays = [Padded(Blab, a) for a in (rp, ci, va, z, r, np.full(L.count, np.nan))]
    d_rp, d_ci, d_va, dz, dr, dc = arrays
    try:
        a = Blab.AmgStageArgs(rows=len(rp) - 1, cols=L.cols, coarse_rows=L.count, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr,
                              agg_ptr=fixed[0].ptr, members=fixed[1].ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
        assert Blab.amg_stage("residual_restrict", a) == 0
        got = dc.read()
        for dev, host in zip(arrays[:5] + list(fixed), (rp, ci, va, z, r, L.agg_ptr, L.members)):
            assert np.array_equal(dev.read().view(np.uint8), np.ascontiguousarray(host).view(np.uint8)), "an input was written"
        return got
    finally:
        for d in arrays:
            d.free()


@pytest.mark.parametrize("planter", P.AGG_PLANTERS)
def test_residual_restrict_under_poison(Blab, planter):
    """Every target and slot of the planter: r_c is the reference's as a NaN class (so +-inf and +-0.0 are exact), and every coarse
    row whose inputs are the clean level's has the bits of the clean run of the same level."""
    L = P.aggregate_level()
    fixed = [Padded(Blab, L.agg_ptr), Padded(Blab, L.members)]
    try:
        clean = run_restrict(Blab, L, L.rp, L.ci, L.va, L.z, L.r, fixed)
        assert same_bits(clean, P.aggregate_reference())
        for case in P.aggregate_cases(planter):
            c, want = P.aggregate_case(*case), P.aggregate_reference(*case)
            got = run_restrict(Blab, L, c.rp, c.ci, c.va, c.z, c.r, fixed)
            assert same_bits_nan_as_class(got, want), case
            outside = np.setdiff1d(np.arange(L.count), c.touched)
            assert same_bits(got[outside], clean[outside]), (case, "a value crossed into another aggregate")
    finally:
        for d in fixed:
            d.free()


# ---------------------------------------------------------------- restriction, batched
@functools.lru_cache(maxsize=None)
def clean_block(k):
    """(Z, R, want): k columns of z and r for aggregate_level(), column k // 2 the level's own z and r, the others standard normal, and
    the reference's coarse block. Built once per k, never written."""
    L = P.aggregate_level()
    rng = np.random.default_rng(2950 + k)
    Z, R = rng.standard_normal((L.cols, k)), rng.standard_normal((len(L.rp) - 1, k))
    Z[:, k // 2], R[:, k // 2] = L.z, L.r
    want = reference_block(L.rp, L.ci, L.va, Z, R)
    for a in (Z, R, want):
        a.setflags(write=False)
    return Z, R, want


def reference_block(rp, ci, va, Z, R):
    from oracle import oracle as O

    L = P.aggregate_level()
    g = AMG.Aggregates(L.count, L.agg, L.agg_ptr, L.members)
    with np.errstate(invalid="ignore"):
        return np.stack([AMG.restrict(O.axpy(-1.0, O.spmv_csr(rp, ci, va, np.ascontiguousarray(Z[:, j])), np.ascontiguousarray(R[:, j])), g)
                         for j in range(Z.shape[1])], axis=1)


def run_restrict_multi(Blab, L, k, rp, ci, va, Z, R, fixed, shift):
    hold = holder(Blab, shift)
    csr = [Padded(Blab, a) for a in (rp, ci, va)]
    blocks = [hold(Z.reshape(-1)), hold(R.reshape(-1)), hold(np.full(L.count * k, np.nan))]
    try:
        a = Blab.AmgStageArgs(rows=len(rp) - 1, cols=L.cols, coarse_rows=L.count, row_ptr=csr[0].ptr, col_idx=csr[1].ptr, values=csr[2].ptr,
                              agg_ptr=fixed[0].ptr, members=fixed[1].ptr, z=blocks[0].ptr, r=blocks[1].ptr, coarse=blocks[2].ptr)
        assert Blab.amg_multi_stage("residual_restrict", k, a) == 0
        got = blocks[2].read().reshape(L.count, k)
        for dev, host in zip(csr + list(fixed), (rp, ci, va, L.agg_ptr, L.members)):
            assert np.array_equal(dev.read().view(np.uint8), np.ascontiguousarray(host).view(np.uint8)), "an input was written"
        assert same_bits(blocks[0].read(), Z.reshape(-1)) and same_bits(blocks[1].read(), R.reshape(-1)), "an input was written"
        return got
    finally:
        for d in csr + blocks:
            d.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("planter", P.AGG_PLANTERS)
def test_residual_restrict_multi_under_poison(Blab, planter, k):
    """The poisoned z and r sit in column k // 2 only. That column is its reference's as a NaN class, and outside the touched coarse
    rows it has the clean run's bits; every other column has its clean bits everywhere but at the target, where the case's matrix
    (an inf coefficient, emptied rows) reaches it as that column's own reference says. Odd k: once more with the block vectors 8
    bytes off a 16-byte boundary."""
    L = P.aggregate_level()
    sick = k // 2
    Zc, Rc, want_clean = clean_block(k)
    fixed = [Padded(Blab, L.agg_ptr), Padded(Blab, L.members)]
    try:
        for shift in shifts_of(k):
            clean = run_restrict_multi(Blab, L, k, L.rp, L.ci, L.va, Zc, Rc, fixed, shift)
            assert same_bits(clean, want_clean), (k, shift)
            for case in P.aggregate_cases(planter):
                c = P.aggregate_case(*case)
                I = P.coarse_of(case[1])
                Z, R = Zc.copy(), Rc.copy()
                Z[:, sick], R[:, sick] = c.z, c.r
                same_matrix = planter in ("r_inf", "z_inf")
                want = reference_block(c.rp, c.ci, c.va, Z, R)
                got = run_restrict_multi(Blab, L, k, c.rp, c.ci, c.va, Z, R, fixed, shift)
                assert same_bits_nan_as_class(got, want), (case, k, shift)
                assert same_bits_nan_as_class(got[:, sick], P.aggregate_reference(*case)), (case, k, shift)
                outside = np.setdiff1d(np.arange(L.count), c.touched)
                assert same_bits(got[outside, sick], clean[outside, sick]), (case, k, shift, "a value crossed into another aggregate")
                others = [j for j in range(k) if j != sick]
                rest = np.arange(L.count) != I
                assert same_bits(got[rest][:, others], clean[rest][:, others]), (case, k, shift, "a value crossed into another column")
                if same_matrix:
                    assert same_bits(got[:, others], clean[:, others]), (case, k, shift, "a value crossed into another column")
                elif planter == "coef_inf" and others:
                    assert not np.isfinite(want[I, others]).any()  # the matrix's poison reaches every column
    finally:
        for d in fixed:
            d.free()


# ---------------------------------------------------------------- prolongation
@pytest.mark.parametrize("rows", P.PROLONG_ROWS)
def test_prolong_correct_under_poison(Blab, O, rows):
    """+inf in e_c at aggregate I appears exactly at the rows with agg == I, everything else has the clean run's bits; e_c = z = -0.0
    gives -0.0; e_c and agg keep their bits."""
    L = P.prolong_level(rows)
    d_agg = Padded(Blab, L.agg)
    try:
        def run(ec, z):
            dz, de = Padded(Blab, z), Padded(Blab, ec)
            try:
                a = Blab.AmgStageArgs(rows=rows, coarse_rows=L.coarse_rows, agg=d_agg.ptr, z=dz.ptr, coarse=de.ptr)
                assert Blab.amg_stage("prolong_correct", a) == 0
                got = dz.read()
                assert same_bits(de.read(), ec) and np.array_equal(d_agg.read(), L.agg), "an input was written"
                return got
            finally:
                dz.free(), de.free()

        clean = run(L.ec, L.z)
        assert same_bits(clean, O.axpy(2.0, np.ascontiguousarray(L.ec[L.agg]), L.z))
        for label, ec, z, I in P.prolong_cases(rows):
            got = run(ec, z)
            assert same_bits_nan_as_class(got, O.axpy(2.0, np.ascontiguousarray(ec[L.agg]), z)), (rows, label)
            if I is None:
                assert same_bits(got, np.full(rows, -0.0)), (rows, label)
            else:
                hit = L.agg == I
                assert hit.any() and same_bits(got[hit], np.full(int(hit.sum()), np.inf)) and same_bits(got[~hit], clean[~hit]), (rows, label)
    finally:
        d_agg.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", P.PROLONG_ROWS)
def test_prolong_correct_multi_under_poison(Blab, O, rows, k):
    """The same on blocks of k columns with the poison in column k // 2 only: the other columns keep their clean bits. Odd k: once
    more 8 bytes off a 16-byte boundary."""
    L = P.prolong_level(rows)
    sick = k // 2
    rng = np.random.default_rng(7200 + 10 * rows + k)
    Zc, Ec = rng.standard_normal((rows, k)), rng.standard_normal((L.coarse_rows, k))
    Zc[:, sick], Ec[:, sick] = L.z, L.ec
    d_agg = Padded(Blab, L.agg)
    try:
        for shift in shifts_of(k):
            hold = holder(Blab, shift)

            def run(E, Z):
                dz, de = hold(Z.reshape(-1)), hold(E.reshape(-1))
                try:
                    a = Blab.AmgStageArgs(rows=rows, coarse_rows=L.coarse_rows, agg=d_agg.ptr, z=dz.ptr, coarse=de.ptr)
                    assert Blab.amg_multi_stage("prolong_correct", k, a) == 0
                    got = dz.read().reshape(rows, k)
                    assert same_bits(de.read(), E.reshape(-1)) and np.array_equal(d_agg.read(), L.agg), "an input was written"
                    return got
                finally:
                    dz.free(), de.free()

            clean = run(Ec, Zc)
            for j in range(k):
                assert same_bits(clean[:, j], O.axpy(2.0, np.ascontiguousarray(Ec[L.agg, j]), np.ascontiguousarray(Zc[:, j]))), (rows, k, j)
            for label, ec, z, I in P.prolong_cases(rows):
                E, Z = Ec.copy(), Zc.copy()
                E[:, sick], Z[:, sick] = ec, z
                got = run(E, Z)
                others = [j for j in range(k) if j != sick]
                assert same_bits(got[:, others], clean[:, others]), (rows, k, label, shift, "a value crossed into another column")
                assert same_bits_nan_as_class(got[:, sick], O.axpy(2.0, np.ascontiguousarray(ec[L.agg]), z)), (rows, k, label, shift)
                if I is None:
                    assert same_bits(got[:, sick], np.full(rows, -0.0)), (rows, k, label, shift)
                else:
                    hit = L.agg == I
                    assert same_bits(got[hit, sick], np.full(int(hit.sum()), np.inf)) and same_bits(got[~hit, sick], clean[~hit, sick]), (rows, k, label)
    finally:
        d_agg.free()


# ---------------------------------------------------------------- the CSR operator: block product and fused partials
@functools.lru_cache(maxsize=None)
def csr_system(name):
    """(rp, ci, va, n, x, x_poisoned, x_at, rows_hit): CR.table_square() with +inf at the table's reserved columns, or CR.arrow(3000)
    with +inf at five columns that are no hub's -- the first two, both sides of the first seam between logical blocks, the last --;
    rows_hit is the matrix's adjacency of the poison (P.poisoned_rows). Built once, never written."""
    if name == "table-square":
        rp, ci, va = CR.table_square()
        t = CR.adaptive_table()
        n, x, xp, x_at = len(rp) - 1, t.x, t.x_poisoned, t.reserved
    else:
        a = CR.arrow(int(name.split("-")[1]))
        rp, ci, va, n = a.rp, a.ci, a.va, a.n
        x = np.random.default_rng(len(ci)).standard_normal(n)
        free = [j for j in range(n) if j not in a.hubs]
        x_at = np.array(sorted({free[0], free[1], a.per_block - 1, a.per_block, free[-1]} - set(a.hubs)), dtype=np.int64)
        xp = x.copy()
        xp[x_at] = np.inf
    rows_hit = P.poisoned_rows(rp, ci, x_at, [])
    assert 0 < len(rows_hit) < n // 10
    for v in (x, xp, x_at, rows_hit):
        v.setflags(write=False)
    return rp, ci, va, n, x, xp, x_at, rows_hit


def open_csr(Bx, rp, ci, va, n, entries=None):
    Bx.lib().spmv_amd_reset_host_matrices()
    m = Bx.HostMatrix(CR.entries_of(rp, ci, va) if entries is None else entries, n, n, -1)
    op = Bx.Operator("cusparse-csr")
    op.select_variant(None)
    assert op.init(m) == 0
    return op, m


def close_csr(op):
    op.free()
    op.select_variant(None)


@pytest.mark.parametrize("name", ["table-square", "arrow-3000"])
def test_spmm_csr_rows_and_columns(B, O, name):
    """spmv_amd_spmm_device on cusparse-csr ("spmm/csr"): +inf in one column of the block at columns only known rows hold. Row
    isolation: that column is the oracle's product as a NaN class, non-finite exactly at the matrix's adjacency of the poison. Column
    isolation: the other columns are bit-equal to their own products."""
    rp, ci, va, n, x, xp, x_at, rows_hit = csr_system(name)
    with np.errstate(invalid="ignore"):
        want_p = O.spmv_csr(rp, ci, va, xp)
    assert np.array_equal(np.flatnonzero(~np.isfinite(want_p)), rows_hit)
    clean = np.random.default_rng(4100 + n).standard_normal((8, n))
    want_clean = [O.spmv_csr(rp, ci, va, clean[j]) for j in range(8)]
    op, _ = open_csr(B, rp, ci, va, n)
    multi = B._multi_lib()
    try:
        for k in KS:
            X = clean[:k].copy()
            X[k // 2] = xp
            xb = interleaved(X, k)
            for shift in shifts_of(k):
                hold = holder(B, shift)
                dx, dy = hold(xb), hold(np.full(n * k, np.nan))
                try:
                    assert multi.spmv_amd_spmm_device(b"cusparse-csr", k, dx.ptr, dy.ptr) == 0
                    assert op.spmm_variant() == "spmm/csr"
                    got = dy.read()
                    for j in range(k):
                        gj = column(got, k, j)
                        if j == k // 2:
                            assert same_bits_nan_as_class(gj, want_p), (name, k, j, shift)
                        else:
                            assert same_bits(gj, want_clean[j]), (name, k, j, shift, "a value crossed into another column")
                    assert same_bits(dx.read(), xb)
                finally:
                    dx.free(), dy.free()
    finally:
        close_csr(op)


@pytest.mark.parametrize("name", ["table-square", "arrow-3000"])
def test_fused_partials_under_poison(Blab, name):
    """Blab.fused_spmv under csr/stream and csr/adaptive with +inf in x: y is the restated row sums as a NaN class; the partial of a
    logical block is non-finite exactly when the block holds a row of the poison's adjacency or a row whose own x[row] is poisoned,
    and is CR.stream_block_partials of the poisoned y as a NaN class; every other partial has the bits of the finite run."""
    rp, ci, va, n, x, xp, x_at, rows_hit = csr_system(name)
    per_block, blocks = CR.stream_geometry(n, len(ci))
    sick_blocks = np.unique(np.concatenate([rows_hit, x_at]) // per_block)
    assert 0 < len(sick_blocks) < blocks // 2
    op, _ = open_csr(Blab, rp, ci, va, n)
    try:
        for variant in ("stream", "adaptive"):
            assert op.select_variant(variant) == 0 and op.variant() == "csr/" + variant
            with np.errstate(invalid="ignore"):
                y_p = CR.row_sums(rp, ci, va, xp, variant)
                want_p = CR.stream_block_partials(xp, y_p, per_block)
            assert np.array_equal(np.flatnonzero(~np.isfinite(y_p)), rows_hit)
            assert np.array_equal(np.flatnonzero(~np.isfinite(want_p)), sick_blocks), (name, variant)
            for shift in (0, 1):
                hold = holder(Blab, shift)
                out = {}
                for label, v in (("finite", x), ("poisoned", xp)):
                    dx, dy, dp = hold(v), hold(np.full(n, np.nan)), hold(np.full(blocks, np.nan))
                    try:
                        rc, count = Blab.fused_spmv(op, dx, dy, dp, blocks)
                        assert rc == 0 and count == blocks, (name, variant, label, rc, count)
                        out[label] = (dy.read(), dp.read())
                        assert same_bits(dx.read(), v)
                    finally:
                        dx.free(), dy.free(), dp.free()
                (y0, p0), (y1, p1) = out["finite"], out["poisoned"]
                assert same_bits(y0, CR.row_sums(rp, ci, va, x, variant)) and same_bits(p0, CR.stream_block_partials(x, y0, per_block))
                assert same_bits_nan_as_class(y1, y_p), (name, variant, shift)
                assert same_bits_nan_as_class(p1, want_p), (name, variant, shift)
                assert np.array_equal(np.flatnonzero(~np.isfinite(p1)), sick_blocks), (name, variant, shift)
                well = np.setdiff1d(np.arange(blocks), sick_blocks)
                assert same_bits(p1[well], p0[well]), (name, variant, shift, "a poisoned row's product left its logical block")
                fine = np.setdiff1d(np.arange(n), rows_hit)
                assert same_bits(y1[fine], y0[fine]), (name, variant, shift)
    finally:
        close_csr(op)


# ---------------------------------------------------------------- the CSR a file gives: set-up, application, solves
def check_hierarchy(Blab, M, entries, label):
    """cusparse-csr initialised from `entries`: level 0 is M with its duplicates; every level's aggregates, CSR, dinv and lambda_max
    are the restatement's bit for bit. Returns the restatement's levels at nu = 1."""
    rows = AMG.rows_of(M)
    op, _ = open_csr(Blab, M.rp, M.ci, M.va, rows, entries)
    try:
        pc = Blab.Precond.amg(op, 1)
        levels = AMG.hierarchy(M, 1)
        info = pc.amg_info()
        assert info["rows"] == [L.rows for L in levels] and info["nnz"] == [len(L.M.ci) for L in levels], (label, info)
        for l, L in enumerate(levels):
            rp, ci, va, dinv, agg = pc.amg_level(l)
            assert np.array_equal(rp, L.M.rp) and np.array_equal(ci, L.M.ci), (label, l)
            assert same_bits(va, L.M.va), (label, l, int(np.sum(va != L.M.va)))
            assert same_bits(dinv, L.dinv), (label, l)
            assert same_bits([info["lambda_max"][l]], [L.lambda_max]), (label, l, info["lambda_max"][l], L.lambda_max)
            assert (agg is None) == (L.g is None) and (agg is None or np.array_equal(agg, L.g.agg)), (label, l)
        rp, ci, va, _, _ = pc.amg_level(0)  # the duplicates survive in the CSR the device holds
        same = (np.repeat(np.arange(rows), np.diff(rp))[1:] == np.repeat(np.arange(rows), np.diff(rp))[:-1]) & (ci[1:] == ci[:-1])
        assert int(same.sum()) > 1000 and len(ci) == len(M.ci) and int((va == 0.0).sum()) > 500, label
        pc.destroy()
        return levels
    finally:
        close_csr(op)


def shuffled(name, seed):
    """(M as the device must hold it, the shuffled COO entries it is loaded from)."""
    src = AMG.as_a_file_gives_it(name)
    e = P.shuffled_entries(src.rp, src.ci, src.va, seed)
    return AMG.Csr(*P.csr_of_entries(e, AMG.rows_of(src))), e


def test_split33_from_shuffled_entries(B, Blab, O):
    """split33 loaded from COO entries in shuffled order: the hierarchy, one application at nu = 1 and a whole PCG solve bit for bit
    against the restatement on the CSR a stable sort makes of those entries; the count is the table's."""
    M, e = shuffled("split33", 41)
    rows = AMG.rows_of(M)
    levels = check_hierarchy(Blab, M, e, "split33 shuffled")
    st = AMG.structure(M)
    assert [AMG.rows_of(m) for m, _ in st] == AMG.LEVEL_ROWS["split33"]
    op, m = open_csr(B, M.rp, M.ci, M.va, rows, e)
    try:
        pc = B.Precond.amg(op, 1)
        cycle = AMG.exact_cycle(O, levels, op.variant())
        r = np.random.default_rng(rows + 1).standard_normal(rows)
        dr, dz = Padded(B, r), Padded(B, np.full(rows, np.nan))
        pc.apply_device(op, dr.ptr, dz.ptr)
        assert same_bits(dz.read(), cycle(r)) and same_bits(dr.read(), r)
        dr.free(), dz.free()
        b, x0 = AMG.vectors("split33")
        xo, ho, ito, conv = AMG.pcg_exact(O, M, cycle, b, x0, variant0=op.variant())
        x, h, stats = B.pcg_solve_device(op, m, pc, b, x0)
        wanted = {(n, v): its for n, v, its in AMG.TABLE}[("split33", 1)]
        assert conv and stats.converged == 1 and stats.iterations == ito == wanted, (stats.iterations, ito, wanted)
        assert same_bits(h, ho) and same_bits(x, xo), int(np.sum(x != xo))
        pc.destroy()
    finally:
        close_csr(op)


def test_split33_from_a_matrix_market_file(Blab, O, tmp_path):
    """split33 written to a Matrix Market file in CSR order and read by load_matrix_market: the device holds the file's CSR, duplicates
    and stored zeros in file order, and builds the restatement's hierarchy from it."""
    M = AMG.as_a_file_gives_it("split33")
    rows = AMG.rows_of(M)
    path = tmp_path / "split33.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{rows} {rows} {len(M.ci)}\n")
        for i, j, v in zip(AMG.row_index(M), M.ci, M.va):
            f.write(f"{i + 1} {j + 1} {float(v)!r}\n")
    m = Blab.load_matrix_market(str(path))
    assert (m.c.rows, m.c.cols, len(m.entries)) == (rows, rows, len(M.ci))
    check_hierarchy(Blab, M, m.entries, "split33 file")


def test_oneway33_from_shuffled_entries(B, Blab, O):
    """oneway33 -- cancelling pairs, one-way entries -- from shuffled COO entries: the hierarchy, one application and GCR(16) bit for
    bit; the count is the stored one."""
    name, nu, restart, iterations = AMG.GCR_ROW_ONEWAY
    M, e = shuffled(name, 42)
    rows = AMG.rows_of(M)
    levels = check_hierarchy(Blab, M, e, "oneway33 shuffled")
    assert [L.rows for L in levels] == [1089, 198, 30]
    _, b, x0 = AMG.oneway33()
    op, m = open_csr(B, M.rp, M.ci, M.va, rows, e)
    try:
        pc = B.Precond.amg(op, nu)
        cycle = AMG.exact_cycle(O, levels, op.variant())
        dr, dz = Padded(B, b), Padded(B, np.full(rows, np.nan))
        pc.apply_device(op, dr.ptr, dz.ptr)
        assert same_bits(dz.read(), cycle(b)) and same_bits(dr.read(), b)
        dr.free(), dz.free()
        want = GR.gcr_exact(lambda v: O.spmv_csr(M.rp, M.ci, M.va, v), b, x0, cycle, restart)
        x, h, stats = B.gcr_solve(op, m, pc, b, x0, restart=restart)
        assert stats.converged == 1 and stats.iterations == want[2] == iterations, (stats.iterations, want[2], iterations)
        assert same_bits(h, want[1]) and same_bits(x, want[0])
        pc.destroy()
    finally:
        close_csr(op)


def test_split33_batched_application_carries_the_single_bits(B, O):
    """An amg_multi handle (max_rhs = 3) on split33 from shuffled entries: one batched application, every column with the bits of the
    single-vector application on the same handle and of the restatement."""
    M, e = shuffled("split33", 41)
    rows = AMG.rows_of(M)
    op, _ = open_csr(B, M.rp, M.ci, M.va, rows, e)
    try:
        pc = B.Precond.amg_multi(op, 1, 0, AMG.THETA, 3)
        levels = AMG.hierarchy(M, 1)
        assert pc.amg_info()["rows"] == [L.rows for L in levels] and PA.bits_coincide(levels)
        R = np.random.default_rng(rows + 3).standard_normal((3, rows))
        block = np.ascontiguousarray(R.T).ravel()
        dR, dZ = Guarded(B, block), Guarded(B, np.full(3 * rows, np.nan))
        pc.apply_device_multi(op, 3, dR.ptr, dZ.ptr)
        got = dZ.read().reshape(rows, 3)
        assert same_bits(dR.read(), block)
        dR.free(), dZ.free()
        cycle, single = PA.make_cycle(levels), AMG.exact_cycle(O, levels, op.variant())
        for j in range(3):
            dr, dz = Guarded(B, R[j]), Guarded(B, np.full(rows, np.nan))
            pc.apply_device(op, dr.ptr, dz.ptr)
            z = dz.read()
            dr.free(), dz.free()
            assert same_bits(got[:, j], z), (j, "the batched column differs from the single-vector application")
            assert same_bits(z, single(R[j])) and same_bits(got[:, j], cycle(R[j])), j
        pc.destroy()
    finally:
        close_csr(op)
