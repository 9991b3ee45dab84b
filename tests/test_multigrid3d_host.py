"""The aggregation multigrid preconditioner of the 3-D operator (csrc/multigrid3d.hip), CPU side: the new entry
points are declared, exported and bound; every refusal that needs no device holds before any HIP call; the restatement's coarse
operators are P^T A P and bit-symmetric; its V-cycle is a symmetric operator; and its preconditioned loop takes the table's iteration
counts in two independent roundings, clear of the tolerance and with histories far below the 1e-10 the GPU is held to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import multigrid3d_restatement as M3
import pcg_restatement as P
import stencil7 as S7
from conftest import ROOT

NEW = ["spmv_amd_precond_create_multigrid3d", "spmv_amd_precond_multigrid_dimension", "spmv_amd_init_stencil7_synthetic_values"]
TWO_ROUNDINGS = 1e-12  # what the two roundings' histories may differ by on a table row (tests/test_multigrid_host.py's rule)


def test_multigrid3d_symbols_exported_declared_and_bound(B):
    L = B._pcg_lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS and name not in B.LAB_ONLY_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for method in ("multigrid3d", "multigrid_dimension", "multigrid_level"):
        assert callable(getattr(B.Precond, method)), method


def test_the_lab_only_stages_are_absent_from_the_product_library(B):
    """The 3-D stages are names spmv_amd_mg_stage takes: the product library has neither that entry point nor the level reader."""
    for name in ("spmv_amd_mg_stage", "spmv_amd_precond_multigrid_level_csr", "spmv_amd_pcg_last_multigrid_cycles"):
        assert name in B.LAB_ONLY_SYMBOLS and not hasattr(B.lib(), name), name
    lab = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    for stage in ("coarsen3d", "residual_restrict3d", "prolong3d"):
        assert '"' + stage + '"' in lab, stage
    with pytest.raises(RuntimeError):
        B.mg_stage("coarsen3d", None)


def test_multigrid3d_refuses_without_touching_the_gpu(B):
    for mode in ("stencil7-csr", "stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()  # free() of an operator that was never initialised touches no device memory
    L = B._pcg_lib()
    bad = C.c_int(7)
    stencil7 = B.Operator("stencil7-csr").op

    def refused(op, nu, max_levels, bad_row=bad):
        bad.value = 7
        got = L.spmv_amd_precond_create_multigrid3d(op, nu, max_levels, None if bad_row is None else C.byref(bad_row))
        return not got and (bad_row is None or bad.value == -1)

    assert refused(None, 1, 0)
    for nu in (-1, 9, -2 ** 31, 2 ** 31 - 1):
        assert refused(stencil7, nu, 0), nu
    for max_levels in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        assert refused(stencil7, 1, max_levels), max_levels
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):  # not stencil7-csr: refused whether initialised or not
        assert refused(B.Operator(mode).op, 1, 0), mode
    for nu, max_levels in ((0, 0), (1, 1), (8, 32)):  # stencil7-csr used before init
        assert refused(stencil7, nu, max_levels)
    assert refused(stencil7, 1, 0, bad_row=None)  # bad_row may be NULL
    own = B.SpmvOperator()  # a caller's own table, even under the operator's name
    own.name = b"stencil7-csr"
    assert refused(C.pointer(own), 1, 0)
    assert L.spmv_amd_precond_multigrid_dimension(None) == 0


def test_grids_and_members():
    assert M3.grids(130) == [130, 65, 33, 17, 9, 5] and M3.grids(8) == [8] and M3.grids(9) == [9, 5]
    assert M3.grids(66) == [66, 33, 17, 9, 5] and M3.grids(130, 2) == [130, 65]
    assert M3.MEMBERS == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]


def systems_for_the_operators():
    yield "poisson9", M3.poisson(9), 9
    yield "poisson10", M3.poisson(10), 10
    yield "conductance17", M3.conductance_stencil(17, 2), 17
    yield "conductance20", M3.conductance_stencil(20, 1), 20
    yield "generator9", M3.matrix_of(S7.coo(9), 9), 9


def test_coarse_operators_are_galerkin_and_bit_symmetric():
    """Every level against scipy's P^T A P: each entry within 1e-14 of the sum of its terms' magnitudes (a re-ordered sum of at most
    thirty-two terms); the complete 7-point pattern; and, the fine matrix being bit-symmetric, A_c == A_c^T bit for bit."""
    for name, A, n in systems_for_the_operators():
        assert (A != A.T).nnz == 0, name
        for nl in M3.grids(n)[:-1]:
            Ac = M3.coarsen(A, nl)
            nc = (nl + 1) // 2
            Pm = M3.prolongation(nl)
            want = sp.csr_matrix(Pm.T @ A @ Pm)
            scale = sp.csr_matrix(Pm.T @ abs(A) @ Pm)
            want.sort_indices(), scale.sort_indices()
            assert Ac.has_sorted_indices and Ac.nnz == S7.nnz(nc), (name, nl)
            pattern = M3.matrix_of(S7.coo(nc), nc)
            assert np.array_equal(Ac.indptr, pattern.indptr) and np.array_equal(Ac.indices, pattern.indices), (name, nl)
            assert np.array_equal(want.indptr, Ac.indptr) and np.array_equal(want.indices, Ac.indices), (name, nl)
            assert np.all(np.abs(Ac.data - want.data) <= 1e-14 * scale.data), (name, nl)
            At = M3.sorted_csr(Ac.T)
            assert np.array_equal(At.data.view(np.uint64), Ac.data.view(np.uint64)), (name, nl)
            A = Ac


def test_the_cycle_is_symmetric():
    """<u, M^-1 v> = <M^-1 u, v> to 1e-12 of |u| |M^-1 v| on random vectors: nu = 0, 1, 2, even and odd grids, capped hierarchies."""
    rng = np.random.default_rng(17)
    for name, A, n in systems_for_the_operators():
        for nu, max_levels in ((0, 0), (1, 0), (2, 0), (1, 1), (1, 2)):
            apply = M3.make_cycle(M3.hierarchy(A, n, nu, max_levels))
            u, v = rng.standard_normal(n ** 3), rng.standard_normal(n ** 3)
            Mu, Mv = apply(u), apply(v)
            assert abs(u @ Mv - Mu @ v) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv), (name, nu, max_levels)


def test_restrict_and_prolong_are_transposes():
    for n in (9, 10):
        Pm = M3.prolongation(n)
        t = np.random.default_rng(n).standard_normal(n ** 3)
        ec = np.random.default_rng(n + 1).standard_normal(((n + 1) // 2) ** 3)
        assert np.allclose(M3.restrict(t, n), Pm.T @ t, rtol=0, atol=1e-14)
        assert np.array_equal(M3.prolong(ec, n), Pm @ ec)
    # the order of the sum: eight terms of very different magnitude, summed as stated
    t = np.zeros(8)
    t[:] = [1.0, 2.0 ** -53, 2.0 ** -53, 1.0, -2.0, 2.0 ** -30, 3.0, 2.0 ** -52]
    want = 0.0
    for k, v in enumerate(t):
        want = v if k == 0 else want + v
    assert M3.restrict(t, 2)[0] == want


def test_the_cycle_is_the_two_dimensional_one_with_its_own_transfers():
    """make_cycle is multigrid_restatement's code run with this file's restrict and prolong: a one-level hierarchy never calls either
    and gives the 2-D function's result on the same level."""
    import multigrid_restatement as MG
    assert M3.make_cycle.__code__ is MG.make_cycle.__code__
    assert M3.make_cycle.__globals__["restrict"] is M3.restrict and M3.make_cycle.__globals__["prolong"] is M3.prolong
    A = M3.poisson(6)
    levels = M3.hierarchy(A, 6, 1)
    r = np.random.default_rng(1).standard_normal(216)
    assert len(levels) == 1 and np.array_equal(M3.make_cycle(levels)(r), MG.make_cycle(levels)(r))


@pytest.mark.parametrize("name,nu,tol,iterations", M3.TABLE)
def test_table_counts_in_two_roundings(name, nu, tol, iterations):
    A, b, x0, n = M3.table_system(name)
    x1, h1, it1, conv1 = M3.pcg(A, n, b, x0, nu, tol)
    x2, h2, it2, conv2 = M3.pcg_other_rounding(A, n, b, x0, nu, tol)
    err = P.hist_err(h1, h2) if it1 == it2 else float("inf")
    print(f"{name} nu {nu} tol {tol}: {it1} / {it2} iterations, histories {err:.1e} apart, last {h1[-1] / h1[0] / tol:.3f}, "
          f"the one before {h1[-2] / h1[0] / tol:.3f} of tol")
    assert conv1 and conv2 and it1 == it2 == iterations, (name, nu, tol, it1, it2)
    assert err < TWO_ROUNDINGS, (name, nu, tol, err)
    assert M3.row_is_clear(h1, tol) and M3.row_is_clear(h2, tol), (name, nu, tol)
    assert P.true_residual_norm(P.entries_of(A), b, x1) < tol * h1[0] * (1.0 + 1e-6)


def test_the_counts_do_not_grow_like_jacobis():
    """Poisson at nu = 1: 16^3 -> 64^3 takes 6 -> 9 iterations (the issue's prototype: 6 -> 9; Jacobi-PCG 48 -> 163)."""
    ours = {name: its for name, nu, tol, its in M3.TABLE if nu == 1 and tol == 1e-6}
    assert ours["poisson16"] == 6 and ours["poisson64"] == 9
