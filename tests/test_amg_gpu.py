"""The aggregation AMG preconditioner (csrc/amg.hip) on the GPU: the hierarchy the library builds bit for bit
against tests/amg_restatement.py on every matrix of the CPU cases, the application z = M^-1 r bit for bit against the exact form --
under each variant of the operator's product --, whole PCG and GCR solves in the device's bits, refusals and handle lifetime, a clean
solve on the remains of one that ended badly, and the application's --precond=amg."""
import math
import os
import subprocess

import numpy as np
import pytest

import amg_restatement as AMG
import csr_restatement as CSR
import gcr_restatement as GR
import leftovers as LO
from conftest import ROOT
from test_amg_host import SETUP_CASES, same_bits
from test_amg_stages_gpu import Padded

pytestmark = pytest.mark.gpu
SUM_TOL = 1e-13  # a re-ordered fp64 sum against math.fsum, of sum|terms|


@pytest.fixture(autouse=True)
def _gpu(B):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    B.lib().spmv_amd_reset_host_matrices()
    yield
    B.lib().spmv_amd_reset_host_matrices()


def open_csr(Bx, M, variant=None):
    """cusparse-csr holding M, in the automatic variant or a forced one."""
    Bx.lib().spmv_amd_reset_host_matrices()
    rows = AMG.rows_of(M)
    m = Bx.HostMatrix(CSR.entries_of(M.rp, M.ci, M.va), rows, rows, -1)
    op = Bx.Operator("cusparse-csr")
    op.select_variant(variant)
    assert op.init(m) == 0
    return op, m


def close_csr(op):
    op.free()
    op.select_variant(None)


# ---------------------------------------------------------------- hierarchy
@pytest.mark.parametrize("case", SETUP_CASES, ids=[c[0] for c in SETUP_CASES])
def test_hierarchy_bit_for_bit(Blab, case):
    """Every level: the aggregate map equal; the CSR, dinv and lambda_max equal bit for bit; the info's figures."""
    name, make, theta, max_levels = case
    M = make()
    op, _ = open_csr(Blab, M)
    try:
        pc = Blab.Precond.amg(op, 1, max_levels, theta)
        levels = AMG.hierarchy(M, 1, max_levels, theta)
        info = pc.amg_info()
        assert pc.kind == "multigrid" and pc.multigrid_dimension() == 0 and pc.multigrid_max_rhs() == 0 and pc.chebyshev_info() is None
        assert info["rows"] == [L.rows for L in levels] and info["nnz"] == [len(L.M.ci) for L in levels], (name, info)
        assert info["smoother_degree"] == 1 and info["strength"] == theta and info["setup_ms"] > 0.0
        assert info["max_aggregate"] == [0 if L.g is None else int(np.diff(L.g.agg_ptr).max()) for L in levels], name
        nu, grids, lmax = pc.multigrid_info()
        assert nu == 1 and grids == [0] * len(levels) and same_bits(lmax, info["lambda_max"])
        for l, L in enumerate(levels):
            rp, ci, va, dinv, agg = pc.amg_level(l)
            assert np.array_equal(rp, L.M.rp) and np.array_equal(ci, L.M.ci), (name, l)
            assert same_bits(va, L.M.va), (name, l, int(np.sum(va != L.M.va)))
            assert same_bits(dinv, L.dinv), (name, l)
            assert same_bits([info["lambda_max"][l]], [L.lambda_max]), (name, l, info["lambda_max"][l], L.lambda_max)
            assert (agg is None) == (L.g is None) and (agg is None or np.array_equal(agg, L.g.agg)), (name, l)
        assert same_bits(pc.inverse_diagonal(), levels[0].dinv)
        jac = Blab.Precond(op, "jacobi")
        assert jac.amg_info() is None
        jac.destroy()
        pc.destroy()
    finally:
        close_csr(op)


# ---------------------------------------------------------------- application, bit for bit
def check_application(B, O, M, nu, theta, label, forced=None, switch_to=()):
    """apply_device against the exact form under the variant the operator runs; then under each variant of switch_to, chosen by
    spmv_amd_operator_select_variant on the initialised operator with the handle alive."""
    rows = AMG.rows_of(M)
    op, _ = open_csr(B, M, forced)
    try:
        pc = B.Precond.amg(op, nu, 0, theta)
        levels = AMG.hierarchy(M, nu, 0, theta)
        assert pc.amg_info()["rows"] == [L.rows for L in levels], label
        r = np.random.default_rng(rows + nu).standard_normal(rows)
        dr, dz = Padded(B, r), Padded(B, np.full(rows, np.nan))
        seen = []
        for variant in (forced,) + tuple(switch_to):
            if variant is not forced:
                assert op.select_variant(variant) == 0
            running = op.variant()
            seen.append(running)
            z_want = AMG.exact_cycle(O, levels, running)(r)
            rz = pc.apply_device(op, dr.ptr, dz.ptr)
            z = dz.read()
            assert same_bits(z, z_want), (label, running, int(np.sum(z != z_want)), float(np.max(np.abs(z - z_want))))
            assert same_bits(dr.read(), r), label
            terms = r * z_want
            err = abs(rz - math.fsum(terms)) / float(np.sum(np.abs(terms)))
            assert err <= SUM_TOL, (label, running, err)
            again = pc.apply_device(op, dr.ptr, dz.ptr)
            assert again == rz and same_bits(dz.read(), z), (label, running)
        print(f"{label}: variants {seen}, levels {[L.rows for L in levels]}")
        dr.free(), dz.free()
        pc.destroy()
        return seen
    finally:
        close_csr(op)


@pytest.mark.parametrize("name", ["poisson33", "permuted33", "cube9", "nine24", "graph1500"])
def test_application_bit_for_bit(B, O, name):
    M, _ = AMG.system(name)
    for nu in (0, 1, 2):
        assert check_application(B, O, M, nu, AMG.THETA, f"{name} nu {nu}") == ["csr/stream"]


def test_application_on_the_arrow_under_every_variant(B, O):
    """Hub rows of 2 500 entries: the operator runs csr/adaptive by itself; theta = 0 gives levels under aggregates of thousands of
    members (theta = 0.08: one level, the couplings are weak beside the hubs' diagonals). The handle made under the automatic variant
    is applied with the operator switched to adaptive and to wavefront: level 0's product follows the operator, the restriction's
    chain does not."""
    M = AMG.arrow()
    seen = check_application(B, O, M, 1, 0.0, "arrow theta 0", None, ("adaptive", "wavefront", "stream"))
    assert seen == ["csr/adaptive", "csr/adaptive", "csr/wavefront", "csr/stream"]
    check_application(B, O, M, 1, AMG.THETA, "arrow theta 0.08", None, ("wavefront",))


# ---------------------------------------------------------------- whole solves
@pytest.mark.parametrize("name", ["poisson33", "cube9", "nine24", "graph1500"])
@pytest.mark.parametrize("nu", [0, 1])
def test_pcg_bit_for_bit(B, O, name, nu):
    """x, the history and the count against amg_restatement.pcg_exact; the table's count; the same solve twice gives the same bits."""
    M, st = AMG.system(name)
    b, x0 = AMG.vectors(name)
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg(op, nu)
        levels = AMG.hierarchy(M, nu, levels=st)
        xo, ho, ito, conv = AMG.pcg_exact(O, M, AMG.exact_cycle(O, levels, op.variant()), b, x0, variant0=op.variant())
        x, h, stats = B.pcg_solve_device(op, m, pc, b, x0)
        wanted = {(n, v): its for n, v, its in AMG.TABLE}[(name, nu)]
        print(f"{name} nu {nu}: {stats.iterations} iterations (exact form {ito}, table {wanted})")
        assert conv and stats.converged == 1 and stats.iterations == ito == wanted, (name, nu, stats.iterations, ito, wanted)
        assert same_bits(h, ho), (name, nu, [float(v) for v in h[:4]], [float(v) for v in ho[:4]])
        assert same_bits(x, xo), (name, nu, int(np.sum(x != xo)))
        x2, h2, _ = B.pcg_solve_device(op, m, pc, b, x0)
        assert same_bits(x2, x) and same_bits(h2, h), name
        pc.destroy()
    finally:
        close_csr(op)


def test_gcr_on_the_upwind_stencil_bit_for_bit(B, O):
    name, nu, restart, iterations = AMG.GCR_ROW
    M, b, x0 = AMG.upwind33()
    op, m = open_csr(B, M)
    try:
        pc = B.Precond.amg(op, nu)
        levels = AMG.hierarchy(M, nu)
        assert pc.amg_info()["rows"] == [L.rows for L in levels]
        want = GR.gcr_exact(lambda v: O.spmv_csr(M.rp, M.ci, M.va, v), b, x0, AMG.exact_cycle(O, levels, op.variant()), restart)
        x, h, stats = B.gcr_solve(op, m, pc, b, x0, restart=restart)
        assert stats.converged == 1 and stats.iterations == want[2] == iterations, (stats.iterations, want[2])
        assert same_bits(h, want[1]) and same_bits(x, want[0])
        x2, h2, _ = B.gcr_solve(op, m, pc, b, x0, restart=restart)
        assert same_bits(x2, x) and same_bits(h2, h)
        pc.destroy()
    finally:
        close_csr(op)


# ---------------------------------------------------------------- refusals and lifetime
def test_refusals_and_lifetime(B, capfd):
    M, _ = AMG.system("poisson33")
    rows = AMG.rows_of(M)
    b = np.ones(rows)
    op, m = open_csr(B, M)
    try:
        stencil = B.Operator("stencil5-csr")  # initialised, but not cusparse-csr: refused with its name, as before init
        assert stencil.init(B.HostMatrix(CSR.entries_of(M.rp, M.ci, M.va), rows, rows, 33)) == 0
        capfd.readouterr()
        with pytest.raises(ValueError) as info:
            B.Precond.amg(stencil, 1)
        assert info.value.bad_row == -1 and "operator 'stencil5-csr' is not cusparse-csr" in capfd.readouterr().err
        with pytest.raises(ValueError):  # the geometric creator keeps refusing cusparse-csr
            B.Precond.multigrid(op, 1)
        stencil.free()
        pc = B.Precond.amg(op, 1)
        dr, dz = B.DeviceVector.from_host(b), B.DeviceVector(rows, fill=0.0)
        assert pc.apply_device(op, dr.ptr, dz.ptr) != 0.0
        with pytest.raises(RuntimeError):  # d_z == d_r
            pc.apply_device(op, dr.ptr, dr.ptr)
        capfd.readouterr()
        with pytest.raises(RuntimeError):  # BiCGSTAB keeps refusing the kind
            B.bicgstab_solve(op, m, pc, b, np.zeros(rows))
        for batched in (B.pcg_solve_multi, B.gcr_solve_multi, B.bicgstab_solve_multi):  # a hierarchy of single vectors
            capfd.readouterr()
            with pytest.raises(RuntimeError):
                batched(op, m, pc, np.ones((2, rows)), np.zeros((2, rows)))
            if batched is not B.bicgstab_solve_multi:
                assert "keeps single vectors on every level" in capfd.readouterr().err, batched.__name__
        dR, dZ = B.DeviceVector.from_host(np.ones(2 * rows)), B.DeviceVector(2 * rows, fill=0.0)
        with pytest.raises(RuntimeError):
            pc.apply_device_multi(op, 2, dR.ptr, dZ.ptr)
        assert op.init(m) == 0  # a stale handle: made before the operator was last initialised
        with pytest.raises(RuntimeError):
            B.pcg_solve_device(op, m, pc, b, np.zeros(rows))
        with pytest.raises(RuntimeError):
            pc.apply_device(op, dr.ptr, dz.ptr)
        pc.destroy()
        fresh = B.Precond.amg(op, 1)
        _, _, st = B.pcg_solve_device(op, m, fresh, b, np.zeros(rows))
        assert st.converged == 1
        op.free()
        with pytest.raises(RuntimeError):  # after free()
            fresh.apply_device(op, dr.ptr, dz.ptr)
        fresh.destroy()
        for v in (dr, dz, dR, dZ):
            v.free()
    finally:
        close_csr(op)


def test_a_matrix_that_is_not_square_is_refused(B, capfd):
    t = CSR.adaptive_table()
    op = B.Operator("cusparse-csr")
    assert op.init(B.HostMatrix(CSR.entries_of(t.rp, t.ci, t.va), 145, CSR.TABLE_COLS, -1)) == 0
    capfd.readouterr()
    with pytest.raises(ValueError) as info:
        B.Precond.amg(op, 1)
    assert info.value.bad_row == -1 and "a square one is required" in capfd.readouterr().err
    close_csr(op)


def test_a_bad_diagonal_is_refused_with_its_level_and_row(B, capfd):
    """Level 0: a zero diagonal entry. Level 1: 2 x 2 blocks [[1, c], [c, 1]] with c = -0.3 and c = -2 in turn -- each block one
    aggregate, the coarse diagonals 1.4 and -2: row 1 of level 1 has the other sign than row 0's."""
    import scipy.sparse as sp
    M, _ = AMG.system("poisson33")
    va = M.va.copy()
    va[np.nonzero((AMG.row_index(M) == 777) & (M.ci == 777))[0][0]] = 0.0
    op, _ = open_csr(B, AMG.Csr(M.rp, M.ci, va))
    capfd.readouterr()
    with pytest.raises(ValueError) as info:
        B.Precond.amg(op, 1)
    assert info.value.bad_row == 777 and "amg: level 0" in capfd.readouterr().err
    close_csr(op)
    blocks = AMG.csr_of(sp.block_diag([np.array([[1.0, c], [c, 1.0]]) for c in [-0.3, -2.0] * 20]))
    levels = AMG.structure(blocks)
    assert [AMG.rows_of(m) for m, _ in levels] == [80, 40] and np.allclose(AMG.diagonal(levels[1][0])[:2], [1.4, -2.0])
    op, _ = open_csr(B, blocks)
    capfd.readouterr()
    with pytest.raises(ValueError) as info:
        B.Precond.amg(op, 1)
    assert info.value.bad_row == 1 and "amg: level 1" in capfd.readouterr().err
    pc = B.Precond.amg(op, 1, 1)  # one level: the coarse operator is never looked at
    pc.destroy()
    close_csr(op)


# ---------------------------------------------------------------- a clean solve on the remains of one that ended badly
@pytest.mark.parametrize("clean", LO.CLEAN, ids=[c.name for c in LO.CLEAN])
def test_a_solve_inherits_nothing_from_the_one_before(B, clean):
    """The AMG handle over the rows of tests/leftovers.py on the 33 x 33 Poisson matrix in cusparse-csr: behind every dirtying solve
    -- NaN and inf right-hand sides, a zero one, no iterations, huge junk, an early stop --, on the same workspace and the same
    handle, the clean solve gives the bits it gave on a fresh workspace and a fresh handle."""
    grid = 33
    M, _ = AMG.system("poisson33")
    op, m = open_csr(B, M)
    handle = {}

    def solve(d):
        if "pc" not in handle:
            handle["pc"] = B.Precond.amg(op, 1)
        b, x0 = LO.vectors(d, grid, 2)
        x, h, st = B.pcg_solve_device(op, m, handle["pc"], b, x0, max_iters=d.max_iters, tol=d.tol)
        return [LO.column_of(x, h, st)]

    solve.last_history = lambda j, buf: B._pcg_lib().spmv_amd_pcg_last_history(buf.ctypes.data, len(buf))

    def release():
        B.lib().spmv_amd_cg_release_workspace()
        if "pc" in handle:
            handle.pop("pc").destroy()

    try:
        fresh = LO.dirty_then_clean(solve, release, clean, LO.DIRTY)
        assert np.all(np.isfinite(fresh[0].x)) and len(fresh[0].history) == fresh[0].iterations + 1
        if clean.name.startswith("converging"):
            assert fresh[0].converged == 1
    finally:
        release()
        close_csr(op)


# ---------------------------------------------------------------- the application
def test_application_amg_flag(B, O, tmp_path):
    """cg_solver --mode=cusparse-csr --precond=amg on a Matrix Market file of the 24 x 24 9-point stencil, which --precond=multigrid
    refuses: the modes' strings, convergence, and the exact form's count for b = 1."""
    M = AMG.ninepoint(24)
    rows = AMG.rows_of(M)
    path = tmp_path / "nine24.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{rows} {rows} {len(M.ci)}\n")
        for i, j, v in zip(AMG.row_index(M), M.ci, M.va):
            f.write(f"{i + 1} {j + 1} {float(v)!r}\n")
    exe = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")
    levels = AMG.hierarchy(M, 1)
    _, _, want, conv = AMG.pcg_exact(O, M, AMG.exact_cycle(O, levels), np.ones(rows), np.zeros(rows))
    assert conv
    for flags, tag in ((["--precond=amg"], "cusparse-csr+amg1"), (["--precond=amg:2"], "cusparse-csr+amg2"),
                       (["--precond=amg", "--solver=gcr:4"], "cusparse-csr+amg1+gcr4")):
        out = subprocess.run([exe, str(path), "--mode=cusparse-csr"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert f"--- Results for {tag} ---\nConverged: YES in " in out.stdout, out.stdout
        if tag == "cusparse-csr+amg1":
            assert f"Converged: YES in {want} iterations" in out.stdout, (want, out.stdout)
    out = subprocess.run([exe, str(path), "--mode=cusparse-csr", "--precond=multigrid"], capture_output=True, text=True, timeout=300)
    assert "--- Results for" not in out.stdout and "is not stencil5-csr" in out.stderr, (out.stdout, out.stderr)
