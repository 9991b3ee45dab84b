"""The aggregation AMG preconditioner (csrc/amg.hip, csrc/amg_setup.hpp), CPU side: the new entry points are
declared, exported and bound; every refusal that needs no device holds before any HIP call with its sentence; csrc/amg_setup.hpp,
walked by a stand-alone program under sanitizers, gives the restatement's aggregate maps and coarse matrices bit for bit; the
restatement's cycle is a symmetric operator with a positive spectrum; and its preconditioned loops take the table's iteration counts
in two independent roundings, at most half the Jacobi counts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_restatement as AMG
import gcr_restatement as GR
from conftest import ROOT

NEW = ["spmv_amd_precond_create_amg", "spmv_amd_precond_amg_info"]
NEW_LAB = ["spmv_amd_amg_stage", "spmv_amd_precond_amg_level_aggregates"]
EXE = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "bin", "cg_solver")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_amg_symbols_exported_declared_and_bound(B):
    L = B._pcg_lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    lab = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    exports_lab = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports_lab.txt")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS and name not in B.LAB_ONLY_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in NEW_LAB:
        assert name in B.LAB_ONLY_SYMBOLS and not hasattr(B.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", lab) and not re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports_lab, flags=re.M) and not re.search(r"^\s+" + name + r";", exports, flags=re.M), name
    for method in ("amg", "amg_info", "amg_level"):
        assert callable(getattr(B.Precond, method)), method
    assert callable(B.amg_stage)


def test_amg_refuses_without_touching_the_gpu(B, capfd):
    """Every argument and operator check of the creator, each with its one sentence and *bad_row = -1; none reaches a HIP call."""
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()  # free() of an operator that was never initialised touches no device memory
    L = B._pcg_lib()
    bad = C.c_int(7)
    csr = B.Operator("cusparse-csr").op

    def refused(word, op, nu=1, max_levels=0, strength=0.08, bad_row=bad):
        bad.value = 7
        capfd.readouterr()
        got = L.spmv_amd_precond_create_amg(op, nu, max_levels, strength, None if bad_row is None else C.byref(bad_row))
        err = capfd.readouterr().err
        assert not got and (bad_row is None or bad.value == -1), (word, got, bad.value)
        assert "[PCG]" in err and word in err and err.count("\n") == 1, (word, err)

    refused("null operator", None)
    for nu in (-1, 9, -2 ** 31, 2 ** 31 - 1):
        refused("smoother degree", csr, nu=nu)
    for max_levels in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        refused("max_levels", csr, max_levels=max_levels)
    for strength in (float("nan"), float("inf"), float("-inf"), -0.1, 1.0, 7.5):
        refused("strength", csr, strength=strength)
    for mode in ("stencil5-csr", "stencil7-csr", "ellpack", "stencil5-ellpack"):  # not cusparse-csr: the sentence names the operator
        refused(f"operator '{mode}' is not cusparse-csr", B.Operator(mode).op)
    for nu, max_levels, strength in ((0, 0, 0.0), (1, 1, 0.08), (8, 32, 0.99)):  # cusparse-csr used before init
        refused("used before init", csr, nu=nu, max_levels=max_levels, strength=strength)
    refused("used before init", csr, bad_row=None)  # bad_row may be NULL
    own = B.SpmvOperator()  # a caller's own table, even under the operator's name
    own.name = b"cusparse-csr"
    refused("is not cusparse-csr", C.pointer(own))

    levels, nu, theta, ms = C.c_int(-5), C.c_int(-5), C.c_double(-5.0), C.c_double(-5.0)
    rows, lmax = np.full(3, -5, dtype=np.int32), np.full(3, -5.0)
    assert L.spmv_amd_precond_amg_info(None, C.byref(levels), C.byref(nu), C.byref(theta), rows.ctypes.data, None, None, lmax.ctypes.data,
                                       C.byref(ms), 3) == 0
    assert (levels.value, nu.value, theta.value, ms.value) == (-5, -5, -5.0, -5.0) and np.all(rows == -5) and np.all(lmax == -5.0)


def test_amg_stage_refuses_without_touching_the_gpu(Blab, capfd):
    a = Blab.AmgStageArgs(rows=4, cols=4, coarse_rows=2)
    for stage, args, word in (("smooth", a, "unknown"), (None, a, "none named"), ("residual_restrict", None, "null arguments"),
                              ("residual_restrict", a, "CSR array"), ("prolong_correct", a, "aligned"),
                              ("prolong_correct", Blab.AmgStageArgs(rows=0, cols=4, coarse_rows=2), "below 1")):
        capfd.readouterr()
        assert Blab.amg_stage(stage, args) != 0
        err = capfd.readouterr().err
        assert "[PCG] amg: stage" in err and word in err, (stage, word, err)


def test_cg_solver_refuses_amg_where_it_does_not_run():
    """--precond=amg on any mode but cusparse-csr (the default mode included), with --solver=bicgstab, and with a degree out of
    range: one sentence each, before any matrix is built."""
    for args, word in ((["--stencil=16", "--precond=amg"], "--mode=cusparse-csr only"),
                       (["--stencil=16", "--mode=ellpack", "--precond=amg:2"], "--mode=cusparse-csr only"),
                       (["--stencil=16", "--mode=cusparse-csr,stencil5-csr", "--precond=amg"], "--mode=cusparse-csr only"),
                       (["--stencil=16", "--mode=cusparse-csr", "--precond=amg", "--solver=bicgstab"], "--solver=bicgstab takes"),
                       (["--stencil=16", "--mode=cusparse-csr", "--precond=amg:9"], "smoother degree NU of 0..8")):
        out = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and word in out.stderr and out.stderr.count("\n") == 1, (args, out.returncode, out.stderr)
        assert "Matrix loaded" not in out.stdout, args


# ---------------------------------------------------------------- the set-up header against the restatement
def tridiagonal(n):
    return AMG.csr_of(sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]))


def with_lonely_rows():
    """Poisson 12 x 12 and twenty rows that hold their diagonal only, interleaved at the end."""
    return AMG.csr_of(sp.block_diag([AMG.scipy_of(AMG.poisson2d(12)), sp.diags(np.linspace(1.0, 3.0, 20))]))


def heavy_diagonal():
    """Poisson 10 x 10 under a diagonal of 100: no coupling is strong at theta = 0.08."""
    return AMG.csr_of(AMG.scipy_of(AMG.poisson2d(10)) + 96.0 * sp.identity(100))


# (name, matrix, theta, max_levels)
SETUP_CASES = [
    ("poisson33", lambda: AMG.poisson2d(33), AMG.THETA, 0),
    ("cube9", lambda: AMG.poisson3d(9), AMG.THETA, 0),
    ("nine24", lambda: AMG.ninepoint(24), AMG.THETA, 0),
    ("permuted33", lambda: AMG.permuted(AMG.poisson2d(33), 33), AMG.THETA, 0),
    ("arrow3000", AMG.arrow, AMG.THETA, 0),
    ("arrow3000-theta0", AMG.arrow, 0.0, 0),
    ("lonely", with_lonely_rows, AMG.THETA, 0),
    ("tridiagonal69", lambda: tridiagonal(69), AMG.THETA, 0),
    ("poisson8", lambda: AMG.poisson2d(8), AMG.THETA, 0),
    ("heavy", heavy_diagonal, AMG.THETA, 0),
    ("aniso64-theta0", lambda: AMG.poisson2d(64, cy=0.01), 0.0, 0),
    ("poisson33-tie", lambda: AMG.poisson2d(33), 0.25, 0),
    ("poisson33-two-levels", lambda: AMG.poisson2d(33), AMG.THETA, 2),
    ("rectangle", lambda: AMG.poisson2d(40, 13), AMG.THETA, 0),
    # as a file gives them (tests/poison.py): duplicate entries, stored zeros, partly cancelling pairs, one-way entries
    ("split33", lambda: AMG.as_a_file_gives_it("split33"), AMG.THETA, 0),
    ("oneway33", lambda: AMG.as_a_file_gives_it("oneway33"), AMG.THETA, 0),
]


def write_matrix(path, M, theta, max_levels):
    with open(path, "w") as f:
        f.write(f"{AMG.rows_of(M)} {len(M.ci)} {float(theta).hex()} {max_levels}\n")
        f.write(" ".join(str(int(v)) for v in M.rp) + "\n")
        f.write(" ".join(str(int(v)) for v in M.ci) + "\n")
        f.write(" ".join(float(v).hex() for v in M.va) + "\n")


def parse_levels(lines):
    levels = []
    for line in lines:
        words = line.split()
        if words[0] == "level":
            levels.append({"rows": int(words[2]), "nnz": int(words[3]), "count": int(words[4]), "largest": int(words[5])})
        elif words[0] == "va":
            levels[-1]["va"] = np.array([float.fromhex(w) for w in words[1:]], dtype=np.float64)
        else:
            levels[-1][words[0]] = np.array([int(w) for w in words[1:]], dtype=np.int64)
    return levels


@pytest.fixture(scope="module")
def setup_output(tmp_path_factory):
    """tests/abi/amg_setup_test.cpp -- csrc/amg_setup.hpp and standard headers only -- compiled with g++ -fsanitize=address,undefined and
    run once on every case; name -> the printed levels."""
    tmp = tmp_path_factory.mktemp("amg_setup")
    exe = tmp / "amg_setup_test"
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                            "-I", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "amg_setup_test.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    paths = []
    for name, make, theta, max_levels in SETUP_CASES:
        paths.append(str(tmp / f"{name}.txt"))
        write_matrix(paths[-1], make(), theta, max_levels)
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "amg_setup: ok" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    out, current = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("matrix "):
            current = out.setdefault(os.path.basename(line.split()[1])[:-4], [])
        elif not line.startswith("amg_setup:"):
            current.append(line)
    return {name: parse_levels(lines) for name, lines in out.items()}


@pytest.mark.parametrize("case", SETUP_CASES, ids=[c[0] for c in SETUP_CASES])
def test_setup_header_against_the_restatement(setup_output, case):
    """Every level: the same rows, CSR (values bit for bit), aggregate map and member lists."""
    name, make, theta, max_levels = case
    got = setup_output[name]
    want = AMG.structure(make(), max_levels, theta)
    assert [L["rows"] for L in got] == [AMG.rows_of(M) for M, _ in want], name
    for l, (L, (M, g)) in enumerate(zip(got, want)):
        assert np.array_equal(L["rp"], M.rp) and np.array_equal(L["ci"], M.ci), (name, l)
        assert same_bits(L["va"], M.va), (name, l, int(np.sum(L["va"] != M.va)))
        if g is None:
            assert L["count"] == 0 and l == len(got) - 1, (name, l)
            continue
        assert L["count"] == g.count and L["largest"] == int(np.diff(g.agg_ptr).max()), (name, l)
        assert np.array_equal(L["agg"], g.agg) and np.array_equal(L["ptr"], g.agg_ptr) and np.array_equal(L["mem"], g.members), (name, l)


def test_the_cases_are_what_they_are_named_for():
    """The properties the cases were made for, from the restatement alone."""
    rows = {name: [AMG.rows_of(M) for M, _ in AMG.structure(make(), max_levels, theta)] for name, make, theta, max_levels in SETUP_CASES}
    assert rows["poisson33"] == [1089, 195, 28]  # the issue's sketch
    assert rows["poisson8"] == [64]  # 64 rows: one level
    assert rows["heavy"] == [100]  # every row a singleton: 10 n_c > 9 rows, the aggregation is discarded
    assert rows["poisson33-tie"] == [1089]  # v v = 1 = t2 |d_i d_j| at theta = 0.25: the strict > makes nothing strong
    assert not AMG.strong_mask(AMG.poisson2d(33), 0.25).any() and AMG.strong_mask(AMG.poisson2d(33), 0.2499).any()
    assert rows["poisson33-two-levels"] == [1089, 195]
    assert rows["aniso64-theta0"] != [AMG.rows_of(M) for M, _ in AMG.structure(AMG.poisson2d(64, cy=0.01))]  # theta = 0 takes the weak direction too
    # the lonely rows found singletons in pass 3: numbered after every aggregate of the grid
    g = AMG.aggregate(with_lonely_rows())
    assert np.all(np.diff(g.agg_ptr)[g.agg[144:]] == 1) and g.agg[144:].min() > g.agg[:144].max()
    # row 68 of the chain: its one strong neighbour was taken by pass 1, pass 2 places it there
    g = AMG.aggregate(tridiagonal(69))
    assert g.agg[68] == g.agg[67] == g.count - 1 and g.count == 23
    # the arrow's couplings are weak beside its hubs' diagonals: one level at theta = 0.08; at theta = 0 the hub rows make aggregates
    # of thousands (pass 2 sends the spokes to their hub's aggregate)
    assert rows["arrow3000"] == [3000] and len(rows["arrow3000-theta0"]) >= 2
    M, g = AMG.structure(AMG.arrow(), 0, 0.0)[0]
    assert np.diff(g.agg_ptr).max() > 1000


def test_coarse_operators_are_galerkin():
    """Every coarse level against scipy's P^T A P: the same pattern up to stored zeros, each entry within 1e-13 of the sum of its
    terms' magnitudes."""
    for name in ("poisson33", "permuted33", "graph1500", "arrow3000", "nine24"):
        _, levels = AMG.system(name)
        for (Ml, g), (Mc, _) in zip(levels[:-1], levels[1:]):
            n = AMG.rows_of(Ml)
            P = sp.csr_matrix((np.ones(n), (np.arange(n), g.agg)), shape=(n, g.count))
            want = (P.T @ AMG.scipy_of(Ml) @ P).toarray()
            scale = (P.T @ abs(AMG.scipy_of(Ml)) @ P).toarray()
            got = AMG.scipy_of(Mc).toarray()
            assert np.all(np.abs(got - want) <= 1e-13 * scale), name
            assert np.all(np.diff(Mc.rp) >= 1) and all(np.all(np.diff(Mc.ci[Mc.rp[i]:Mc.rp[i + 1]]) > 0) for i in range(g.count)), name


# ---------------------------------------------------------------- the cycle
@pytest.mark.parametrize("name", ["poisson33", "cube9", "nine24"])
def test_the_cycle_is_symmetric_and_positive(name):
    """<u, M^-1 v> = <M^-1 u, v> to 1e-12 of |u| |M^-1 v| at nu = 0, 1, 2, and the spectrum of M^-1 A (dense, nu = 1) is real and
    positive."""
    M, st = AMG.system(name)
    n = AMG.rows_of(M)
    rng = np.random.default_rng(25)
    for nu in (0, 1, 2):
        apply = AMG.make_cycle(AMG.hierarchy(M, nu, levels=st))
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = apply(u), apply(v)
        assert abs(u @ Mv - Mu @ v) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv), (name, nu)
    apply = AMG.make_cycle(AMG.hierarchy(M, 1, levels=st))
    eye = np.eye(n)
    Minv = np.column_stack([apply(eye[:, j]) for j in range(n)])
    Minv = 0.5 * (Minv + Minv.T)
    w = np.linalg.eigvalsh(Minv)
    assert w.min() > 0.0, (name, w.min())  # M^-1 is positive definite, so M^-1 A has the spectrum of A^1/2 M^-1 A^1/2: positive
    spectrum = np.linalg.eigvals(Minv @ AMG.scipy_of(M).toarray())
    print(f"{name}: spectrum of M^-1 A in [{spectrum.real.min():.3f}, {spectrum.real.max():.3f}]")
    assert spectrum.real.min() > 0.0 and np.abs(spectrum.imag).max() <= 1e-9 * spectrum.real.max(), name


def test_restrict_and_prolong_are_transposes():
    M, st = AMG.system("graph1500")
    g = st[0][1]
    n = AMG.rows_of(M)
    P = sp.csr_matrix((np.ones(n), (np.arange(n), g.agg)), shape=(n, g.count))
    t = np.random.default_rng(1).standard_normal(n)
    assert np.allclose(AMG.restrict(t, g), P.T @ t, rtol=0, atol=1e-13)


def test_the_exact_cycle_agrees_with_plain_numpy(O):
    """The exact form -- the variants' row sums, the sequential chain under the restriction, the oracle's fma -- is one more rounding
    of the same cycle: 1e-12 of |z| on the systems the GPU is held to it on."""
    for name in ("poisson33", "cube9", "nine24", "arrow3000"):
        M, st = AMG.system(name)
        levels = AMG.hierarchy(M, 1, levels=st)
        r = np.random.default_rng(3).standard_normal(AMG.rows_of(M))
        z, ze = AMG.make_cycle(levels)(r), AMG.exact_cycle(O, levels)(r)
        assert np.linalg.norm(z - ze) <= 1e-12 * np.linalg.norm(z), name


# ---------------------------------------------------------------- whole solves
def test_the_table_has_the_rows_of_the_issue():
    """Twelve symmetric systems at nu = 0, 1, 2; at most two rows may be missing. None is."""
    assert len({(name, nu) for name, nu, _ in AMG.TABLE}) >= 36 - 2
    assert {name for name, _, _ in AMG.TABLE} == set(AMG.JACOBI)


@pytest.mark.parametrize("name,nu,iterations", AMG.TABLE)
def test_table_counts_in_two_roundings(name, nu, iterations):
    M, st = AMG.system(name)
    assert [AMG.rows_of(m) for m, _ in st] == AMG.LEVEL_ROWS[name]
    b, x0 = AMG.vectors(name)
    levels = AMG.hierarchy(M, nu, levels=st)
    x1, h1, it1, conv1 = AMG.pcg(levels, b, x0)
    x2, h2, it2, conv2 = AMG.pcg_other_rounding(levels, b, x0)
    print(f"{name} nu {nu}: {it1} / {it2} iterations, last {h1[-1] / h1[0]:.3e}")
    assert conv1 and conv2 and it1 == it2 == iterations, (name, nu, it1, it2)
    A = AMG.scipy_of(M)
    assert np.linalg.norm(b - A @ x1) < 1e-6 * h1[0] * (1.0 + 1e-6)


@pytest.mark.parametrize("name", sorted(AMG.JACOBI))
def test_amg_halves_the_jacobi_counts(name):
    """On every symmetric system the nu = 1 count is at most half the Jacobi count of the same restatement (b, x0, tol and loop)."""
    M, _ = AMG.system(name)
    b, x0 = AMG.vectors(name)
    _, _, jacobi, conv = AMG.jacobi_pcg(M, b, x0)
    assert conv and jacobi == AMG.JACOBI[name], (name, jacobi)
    ours = {n: its for n, nu, its in AMG.TABLE if nu == 1}[name]
    assert 2 * ours <= jacobi, (name, ours, jacobi)


def test_gcr_on_the_upwind_stencil_in_two_roundings(O):
    """GCR(16) on the 33 x 33 upwind stencil with the AMG cycle at nu = 1: the stored count in both CPU roundings and in the exact form."""
    name, nu, restart, iterations = AMG.GCR_ROW
    M, b, x0 = AMG.upwind33()
    levels = AMG.hierarchy(M, nu)
    A = AMG.scipy_of(M)
    r1 = GR.gcr(A, b, x0, AMG.make_cycle(levels), restart)
    r2 = GR.gcr_other_rounding(A, b, x0, AMG.other_cycle(levels), restart)
    r3 = GR.gcr_exact(lambda v: O.spmv_csr(M.rp, M.ci, M.va, v), b, x0, AMG.exact_cycle(O, levels), restart)
    assert all(r[2] == iterations and r[3] for r in (r1, r2, r3)), [r[2:4] for r in (r1, r2, r3)]
    assert GR.hist_err(r1[1], r2[1]) < 1e-12 and GR.hist_err(r3[1], r1[1]) < 1e-10


def test_gcr_on_oneway33_in_two_roundings(O):
    """The same on oneway33 -- duplicates, stored zeros, cancelling pairs and a pattern that is not symmetric --: the stored count in
    both CPU roundings and in the exact form."""
    name, nu, restart, iterations = AMG.GCR_ROW_ONEWAY
    M, b, x0 = AMG.oneway33()
    levels = AMG.hierarchy(M, nu)
    assert [L.rows for L in levels] == [1089, 198, 30]
    A = AMG.scipy_of(M)
    r1 = GR.gcr(A, b, x0, AMG.make_cycle(levels), restart)
    r2 = GR.gcr_other_rounding(A, b, x0, AMG.other_cycle(levels), restart)
    r3 = GR.gcr_exact(lambda v: O.spmv_csr(M.rp, M.ci, M.va, v), b, x0, AMG.exact_cycle(O, levels), restart)
    assert all(r[2] == iterations and r[3] for r in (r1, r2, r3)), [r[2:4] for r in (r1, r2, r3)]
    assert GR.hist_err(r1[1], r2[1]) < 1e-12 and GR.hist_err(r3[1], r1[1]) < 1e-10
