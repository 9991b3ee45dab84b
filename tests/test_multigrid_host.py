"""The aggregation multigrid preconditioner (csrc/multigrid.hip), CPU side: the new entry points are declared,
exported and bound; every refusal that needs no device holds before any HIP call; the restatement's coarse operators are P^T A P and
bit-symmetric; its V-cycle is a symmetric operator; and its preconditioned loop takes the table's iteration counts in two independent
roundings whose histories agree far below the 1e-10 the GPU is held to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import chebyshev_restatement as R
import multigrid_restatement as MG
import pcg_restatement as P
from conftest import ROOT

NEW = ["spmv_amd_precond_create_multigrid", "spmv_amd_precond_multigrid_info"]
NEW_LAB = ["spmv_amd_precond_multigrid_level_csr", "spmv_amd_mg_stage", "spmv_amd_pcg_last_multigrid_cycles"]
TWO_ROUNDINGS = 1e-12  # what the two roundings' histories may differ by on a table row: a hundredth of the GPU tests' 1e-10


def test_multigrid_symbols_exported_declared_and_bound(B):
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
    for method in ("multigrid", "multigrid_info", "multigrid_level"):
        assert callable(getattr(B.Precond, method)), method
    assert callable(B.mg_stage)


def test_multigrid_refuses_without_touching_the_gpu(B):
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()  # free() of an operator that was never initialised touches no device memory
    L = B._pcg_lib()
    bad = C.c_int(7)
    stencil = B.Operator("stencil5-csr").op

    def refused(op, nu, max_levels, bad_row=bad):
        bad.value = 7
        got = L.spmv_amd_precond_create_multigrid(op, nu, max_levels, None if bad_row is None else C.byref(bad_row))
        return not got and (bad_row is None or bad.value == -1)

    assert refused(None, 1, 0)
    for nu in (-1, 9, -2 ** 31, 2 ** 31 - 1):
        assert refused(stencil, nu, 0), nu
    for max_levels in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        assert refused(stencil, 1, max_levels), max_levels
    for mode in ("cusparse-csr", "ellpack", "stencil5-ellpack"):  # not stencil5-csr: refused whether initialised or not
        assert refused(B.Operator(mode).op, 1, 0), mode
    for nu, max_levels in ((0, 0), (1, 1), (8, 32)):  # stencil5-csr used before init
        assert refused(stencil, nu, max_levels)
    assert refused(stencil, 1, 0, bad_row=None)  # bad_row may be NULL
    own = B.SpmvOperator()  # a caller's own table, even under the operator's name
    own.name = b"stencil5-csr"
    assert refused(C.pointer(own), 1, 0)

    levels, nu = C.c_int(-5), C.c_int(-5)
    grids, lmax = np.full(3, -5, dtype=np.int32), np.full(3, -5.0)
    assert L.spmv_amd_precond_multigrid_info(None, C.byref(levels), C.byref(nu), grids.ctypes.data, lmax.ctypes.data, 3) == 0
    assert (levels.value, nu.value) == (-5, -5) and np.all(grids == -5) and np.all(lmax == -5.0)  # nothing written

    with pytest.raises(ValueError) as info:  # the generic constructor keeps its known kinds
        B.Precond(B.Operator("stencil5-csr"), "multigrid")
    assert info.value.bad_row == -1


def test_grids():
    assert MG.grids(130) == [130, 65, 33, 17, 9, 5]
    assert MG.grids(8) == [8] and MG.grids(9) == [9, 5] and MG.grids(1) == [1]
    assert MG.grids(2000) == [2000, 1000, 500, 250, 125, 63, 32, 16, 8]
    assert MG.grids(130, 1) == [130] and MG.grids(130, 2) == [130, 65] and MG.grids(130, 32) == MG.grids(130)


def systems_for_the_operators():
    yield "poisson9", MG.sorted_csr(P.stencil5(9, center=4.0)), 9
    yield "poisson10", MG.sorted_csr(P.stencil5(10, center=4.0)), 10
    yield "scaled33", MG.sorted_csr(P.scaled_stencil5(33, 2, 5)), 33
    yield "conductance130", MG.conductance_stencil(130, 1), 130
    yield "conductance17", MG.conductance_stencil(17, 2), 17


def test_coarse_operators_are_galerkin_and_bit_symmetric():
    """Every level against scipy's P^T A P: each entry within 1e-14 of the sum of its terms' magnitudes (a re-ordered sum of at most
    twelve terms); the complete 5-point pattern; and, the fine matrix being bit-symmetric, A_c == A_c^T bit for bit."""
    for name, A, n in systems_for_the_operators():
        assert (A != A.T).nnz == 0, name
        for nl in MG.grids(n)[:-1]:
            Ac = MG.coarsen(A, nl)
            nc = (nl + 1) // 2
            Pm = MG.prolongation(nl)
            want = sp.csr_matrix(Pm.T @ A @ Pm)
            scale = sp.csr_matrix(Pm.T @ abs(A) @ Pm)
            want.sort_indices(), scale.sort_indices()
            I, J = np.divmod(np.arange(nc * nc), nc)
            lengths = 1 + (I > 0) + (I < nc - 1) + (J > 0) + (J < nc - 1)
            assert np.array_equal(np.diff(Ac.indptr), lengths) and Ac.has_sorted_indices, (name, nl)
            assert np.array_equal(want.indptr, Ac.indptr) and np.array_equal(want.indices, Ac.indices), (name, nl)
            assert np.all(np.abs(Ac.data - want.data) <= 1e-14 * scale.data), (name, nl)
            At = MG.sorted_csr(Ac.T)
            assert np.array_equal(At.data.view(np.uint64), Ac.data.view(np.uint64)), (name, nl)
            A = Ac


def test_the_cycle_is_symmetric():
    """<u, M^-1 v> = <M^-1 u, v> to 1e-12 of |u| |M^-1 v| on random vectors: nu = 0, 1, 2, even and odd grids, capped hierarchies."""
    rng = np.random.default_rng(15)
    for name, A, n in systems_for_the_operators():
        for nu, max_levels in ((0, 0), (1, 0), (2, 0), (1, 1), (1, 2)):
            apply = MG.make_cycle(MG.hierarchy(A, n, nu, max_levels))
            u, v = rng.standard_normal(n * n), rng.standard_normal(n * n)
            Mu, Mv = apply(u), apply(v)
            assert abs(u @ Mv - Mu @ v) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv), (name, nu, max_levels)


def test_restrict_and_prolong_are_transposes():
    for n in (9, 10):
        Pm = MG.prolongation(n)
        t = np.random.default_rng(n).standard_normal(n * n)
        ec = np.random.default_rng(n + 1).standard_normal(((n + 1) // 2) ** 2)
        assert np.allclose(MG.restrict(t, n), Pm.T @ t, rtol=0, atol=1e-14)
        assert np.array_equal(MG.prolong(ec, n), Pm @ ec)


@pytest.mark.parametrize("name,nu,tol,iterations", MG.TABLE)
def test_table_counts_in_two_roundings(name, nu, tol, iterations):
    A, b, x0, n = MG.table_system(name)
    x1, h1, it1, conv1 = MG.pcg(A, n, b, x0, nu, tol)
    x2, h2, it2, conv2 = MG.pcg_other_rounding(A, n, b, x0, nu, tol)
    err = P.hist_err(h1, h2) if it1 == it2 else float("inf")
    print(f"{name} nu {nu} tol {tol}: {it1} / {it2} iterations, histories {err:.1e} apart, last {h1[-1] / h1[0]:.3e}")
    assert conv1 and conv2 and it1 == it2 == iterations, (name, nu, tol, it1, it2)
    assert err < TWO_ROUNDINGS, (name, nu, tol, err)
    assert P.true_residual_norm(P.entries_of(A), b, x1) < tol * h1[0] * (1.0 + 1e-6)


def test_multigrid_cuts_the_poisson_counts_tenfold():
    """poisson127 and poisson255 at nu = 1 take at most a tenth of the Jacobi counts in chebyshev_restatement.TABLE."""
    jacobi = {name: its for name, degree, tol, its in R.TABLE if degree is None and tol == 1e-6}
    ours = {name: its for name, nu, tol, its in MG.TABLE if nu == 1 and tol == 1e-6}
    for name in ("poisson127", "poisson255"):
        assert 10 * ours[name] <= jacobi[name], (name, ours[name], jacobi[name])


def test_vcycle_schedule_under_sanitizers(tmp_path):
    """csrc/mg_schedule.hpp -- the one statement of the V-cycle's launch order and of which step writes the r.z partials, walked by the
    single-vector and the batched cycle alike -- needs no HIP: tests/abi/mg_schedule_test.cpp includes it and standard headers only, is
    compiled with g++ -fsanitize=address,undefined and run as it is. Its lines are compared with api.h's steps (1)-(5), restated here:
    levels 1, 2, 3 and 5 x degree 0, 1, 2, the coarsest level solved by degree 8. Exactly one call per cycle carries `last`: the
    final step of level 0 (one level: the last step of the coarsest solve)."""
    import subprocess

    def cycle(l, levels, nu):
        coarsest = l + 1 == levels
        yield l, "term0"  # (1) term 0, then steps 1..nu; the coarsest level: term 0 and eight steps
        for k in range(1, (8 if coarsest else nu) + 1):
            yield l, f"step{k}"
        if coarsest:
            return
        yield l, "restrict"  # (2)
        yield from cycle(l + 1, levels, nu)  # (3)
        yield l, "prolong"  # (4)
        for k in range(0, nu + 1):  # (5) nu + 1 updates: the first with g = c0, h = 0.0, then steps 1..nu
            yield l, f"step{k}"

    cases = [(levels, nu) for levels in (1, 2, 3, 5) for nu in (0, 1, 2)]
    exe = tmp_path / "mg_schedule_test"
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                            "-I", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "mg_schedule_test.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)] + [str(v) for case in cases for v in case], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "mg_schedule: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    got = {}
    for line in run.stdout.splitlines():
        words = line.split()
        if words[0] == "case":
            current = got.setdefault((int(words[1]), int(words[2])), [])
        elif words[0] != "mg_schedule:":
            current.append((int(words[0]), words[1], int(words[2])))
    assert sorted(got) == sorted(cases)
    for levels, nu in cases:
        calls = got[(levels, nu)]
        want = [(l, op, 0) for l, op in cycle(0, levels, nu)]
        want[-1] = want[-1][:2] + (1,)
        assert calls == want, (levels, nu, calls, want)
        assert sum(last for _, _, last in calls) == 1 and calls[-1][0] == 0 and calls[-1][2] == 1, (levels, nu)
        assert calls[-1][1] == ("step8" if levels == 1 else f"step{nu}"), (levels, nu, calls[-1])
