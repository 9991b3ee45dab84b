"""Preconditioned CG, CPU side: the new entry points are exported by the product library, declared in api.h and listed; their
argument checks refuse bad calls before any HIP call (so they hold on a machine without a GPU), and so do those of the LAB
build's spmv_amd_pcg_stage; the numpy restatement the GPU tests compare against agrees with scipy's preconditioned CG, which
pins the yardstick itself; and on every system of the whole-solve table two roundings of the restatement agree far below the
1e-10 the GPU is held to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from conftest import ROOT
from pcg_restatement import (TABLE, diagonal, entries_of, hist_err, pcg, pcg_other_rounding, scaled_stencil5, stencil5, table_system,
                             true_residual_norm)

NEW = ["spmv_amd_precond_create", "spmv_amd_precond_create_from_diagonal", "spmv_amd_precond_destroy", "spmv_amd_precond_kind",
       "spmv_amd_precond_inverse_diagonal", "spmv_amd_pcg_solve_device", "spmv_amd_pcg_last_history", "spmv_amd_pcg_release_workspace"]


def test_pcg_symbols_exported_declared_and_listed(B):
    L = B.lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    assert re.search(r"typedef struct SpmvAmdPrecond SpmvAmdPrecond;", api)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS, name
        assert name not in B.LAB_ONLY_SYMBOLS


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_precond_create_refuses_without_touching_the_gpu(B):
    _free_all(B)
    L = B._pcg_lib()
    bad = C.c_int(7)
    csr = B.Operator("cusparse-csr").op
    for kind in (b"jacobi", b"none"):
        assert not L.spmv_amd_precond_create(None, kind, C.byref(bad)) and bad.value == -1
        for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):  # used before init
            bad.value = 7
            assert not L.spmv_amd_precond_create(B.Operator(mode).op, kind, C.byref(bad)) and bad.value == -1
    for kind in (None, b"", b"ilu0", b"Jacobi"):
        assert not L.spmv_amd_precond_create(csr, kind, C.byref(bad)) and bad.value == -1
    assert not L.spmv_amd_precond_create(csr, b"jacobi", None)                # bad_row may be NULL
    own = B.SpmvOperator()                                                   # a caller's own vtable: no diagonal to read
    own.name = b"mine"
    assert not L.spmv_amd_precond_create(C.pointer(own), b"jacobi", C.byref(bad)) and bad.value == -1
    buf = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert not L.spmv_amd_precond_create_from_diagonal(None, 4, C.byref(bad)) and bad.value == -1
    for n in (0, -1):
        assert not L.spmv_amd_precond_create_from_diagonal(C.cast(buf, C.c_void_p), n, C.byref(bad)) and bad.value == -1
    L.spmv_amd_precond_destroy(None)
    assert L.spmv_amd_precond_kind(None) == b"invalid"
    out = np.zeros(4)
    assert L.spmv_amd_precond_inverse_diagonal(None, out.ctypes.data, 4) != 0


def test_pcg_solve_refuses_without_touching_the_gpu(B):
    _free_all(B)
    L = B._pcg_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    b, x = np.ones(n), np.zeros(n)
    cfg, st = B.CGConfig(10, 1e-6, 0, 0), B.CGStats()
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused before the preconditioner is looked at

    def call(op, pm=None, mat=m.ptr, bb=b.ctypes.data, xx=x.ctypes.data, c=C.byref(cfg), s=C.byref(st)):
        return L.spmv_amd_pcg_solve_device(op, mat, pm, bb, xx, c, s)

    stencil = B.Operator("stencil5-csr").op
    assert call(stencil) != 0                          # no preconditioner
    assert call(None, fake) != 0
    assert call(stencil, fake, mat=None) != 0
    assert call(stencil, fake, bb=None) != 0
    assert call(stencil, fake, xx=None) != 0
    assert call(stencil, fake, c=None) != 0
    assert call(stencil, fake, s=None) != 0
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        assert call(B.Operator(mode).op, fake) != 0    # used before init
    neg = B.CGConfig(-1, 1e-6, 0, 0)
    own = B.SpmvOperator()                             # a caller's vtable without run_device
    own.name = b"mine"
    assert call(C.pointer(own), fake) != 0
    assert call(stencil, fake, c=C.byref(neg)) != 0
    assert np.all(x == 0.0)
    assert L.spmv_amd_pcg_last_history(None, 0) >= 0
    L.spmv_amd_pcg_release_workspace()                 # nothing held: a no-op
    assert B._multi_lib().spmv_amd_cg_multi_workspace_bytes() == 0


def _scipy_pcg(A, b, dinv, tol, max_iters):
    count = [0]

    def cb(_):
        count[0] += 1

    M = None if dinv is None else sp.diags(dinv)
    x, info = sla.cg(A, b, x0=np.zeros_like(b), rtol=tol, atol=0.0, maxiter=max_iters, M=M, callback=cb)
    return x, info, count[0]


def test_restatement_agrees_with_scipy_preconditioned_cg():
    """On the scaled stencils S A S the GPU tests use: same iteration counts and solutions as scipy.sparse.linalg.cg(M=D^-1),
    and the gap the feature is about (d = 2 decades at 128^2: CG needs hundreds of iterations, Jacobi-PCG 24)."""
    for n, decades, seed in ((64, 1, 3), (128, 2, 1)):
        A = scaled_stencil5(n, decades, seed)
        b = np.ones(A.shape[0])
        dinv = 1.0 / diagonal(A)
        for d in (dinv, None):
            x, hist, it, conv = pcg(A, b, np.zeros_like(b), d, 1e-6, 2000)
            xs, info, its = _scipy_pcg(A, b, d, 1e-6, 2000)
            assert conv and info == 0 and it == its, (n, decades, d is None, it, its)
            assert len(hist) == it + 1 and hist[-1] / hist[0] < 1e-6 <= hist[-2] / hist[0]
            assert np.max(np.abs(x - xs)) <= 1e-9 * np.max(np.abs(xs))
    A = scaled_stencil5(128, 2, 1)
    b = np.ones(A.shape[0])
    _, _, it_cg, conv_cg = pcg(A, b, np.zeros_like(b), None, 1e-6, 200)
    _, hist, it_j, conv_j = pcg(A, b, np.zeros_like(b), 1.0 / diagonal(A), 1e-6, 200)
    assert not conv_cg and it_cg == 200
    assert conv_j and it_j == 24
    # the seed keeps the last ratio well away from tol (the value test then cannot flip on a rounding difference)
    assert abs(hist[-1] / hist[0] / 1e-6 - 1.0) > 0.01 and abs(hist[-2] / hist[0] / 1e-6 - 1.0) > 0.01


def test_restatement_on_a_constant_diagonal_is_plain_cg():
    """Jacobi on the benchmark stencil (diagonal +5) is a multiple of the identity: the same iterates as CG."""
    A = stencil5(40)
    b = np.ones(A.shape[0])
    _, h0, i0, _ = pcg(A, b, np.zeros_like(b), None)
    _, h1, i1, _ = pcg(A, b, np.zeros_like(b), np.full(A.shape[0], 0.2))
    assert i0 == i1 and np.max(np.abs(h0 - h1) / h0) < 1e-12


def test_pcg_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_pcg_stage (LAB build, include/spmv_amd/lab.h): an unknown stage or kind, null arguments, n < 1, count < 1, a null
    or misaligned pointer the stage needs -- each refused before any HIP call, non-zero, with a sentence on stderr. The pointers
    are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.PcgStageArgs(n=5, b=good, Ap=good, dinv=good, r=good, p=good, x=good, partials=good, count=3, which=2, tol=1e-6,
                              hist=good, hist_cap=4)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(stage, kind, a, sc, word):
        rc = Blab.pcg_stage(stage, kind, a, sc)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG]" in err and "refused" in err and word in err, (stage, kind, word, rc, err)

    sc = Blab.PcgScalars()
    for stage in (None, "", "Init", "update", "step"):
        refused(stage, "jacobi", args(), sc, "stage")
    needs = {"init": ("b", "Ap", "dinv", "r", "p"), "update_r": ("Ap", "dinv", "r"), "update_xp": ("r", "dinv", "p", "x")}
    for stage, vectors in needs.items():
        refused(stage, "jacobi", None, sc, "null arguments")
        for kind in (None, "", "ilu0", "Jacobi"):
            refused(stage, kind, args(), sc, "kind")
        for n in (0,):
            refused(stage, "jacobi", args(n=n), sc, "n < 1")
        for name in vectors:
            for kind in ("jacobi", "none"):
                if name == "dinv" and kind == "none":
                    continue  # not looked at
                refused(stage, kind, args(**{name: None}), sc, name + " is null")
                refused(stage, kind, args(**{name: odd}), sc, name + " is not 16-byte aligned")
        if stage != "update_xp":
            refused(stage, "none", args(partials=None), sc, "partials is null")
            refused(stage, "none", args(partials=crooked), sc, "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, "none", args(), None, "scalar record")
    refused("reduce", None, None, sc, "null arguments")
    refused("reduce", None, args(), None, "scalar record")
    for count in (0, -1):
        refused("reduce", None, args(count=count), sc, "count < 1")
    for which in (-1, 3):
        refused("reduce", None, args(which=which), sc, "which")
    refused("reduce", None, args(hist_cap=-1), sc, "hist_cap")
    refused("reduce", None, args(partials=None), sc, "partials is null")
    refused("reduce", None, args(partials=crooked), sc, "partials is not 8-byte aligned")
    refused("reduce", None, args(hist=None), sc, "hist is null")
    refused("reduce", None, args(hist=crooked), sc, "hist is not 8-byte aligned")
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        __import__("conftest").load_binding().pcg_stage("reduce", None, args(), sc)


def test_the_table_of_whole_solve_inputs_holds_in_two_roundings():
    """Every system tests/test_pcg_gpu.py solves from a non-zero first guess, in the restatement (row-order products, numpy dot
    products) and in pcg_other_rounding (column-order products, long-double dot products): equal iteration counts -- the ones the
    table records --, histories within 1e-12 and solutions within 1e-12 (1e-11 where kind none meets a scaled matrix). So 1e-10 against the restatement is a property of these inputs and
    not of one summation order; an input that fails here must not be given to the GPU at 1e-10. The restatement's own distance
    between recursive and true residual stays below what the GPU test's floor and factor assume."""
    systems = {}
    for name, kind, tol, max_iters, iterations in TABLE:
        if name not in systems:
            systems[name] = table_system(name)
        A, b, x0 = systems[name]
        dinv = 1.0 / diagonal(A) if kind == "jacobi" else None
        x1, h1, i1, c1 = pcg(A, b, x0, dinv, tol, max_iters)
        x2, h2, i2, c2 = pcg_other_rounding(A, b, x0, dinv, tol, max_iters)
        case = (name, kind, tol)
        assert i1 == i2 == iterations and c1 == c2 == (max_iters == 1000), (case, i1, i2)
        assert len(h1) == len(h2) == iterations + 1 and hist_err(h1, h2) < 1e-12, (case, hist_err(h1, h2))
        # x: 1e-12 too, except kind none on a scaled matrix, whose x carries the unpreconditioned system's conditioning: the two
        # roundings differ by 2.5e-12 (scaled600, 92 iterations) and 8.5e-12 (scaled127, capped at 40) there, so 1e-11
        x_bound = 1e-11 if kind == "none" and name.startswith("scaled") else 1e-12
        assert np.max(np.abs(x1 - x2)) <= x_bound * np.max(np.abs(x1)), (case, np.max(np.abs(x1 - x2)) / np.max(np.abs(x1)))
        if c1:
            # the converging ratio is not a rounding error away from tol, and the recursive residual is the true one
            assert abs(h1[-1] / h1[0] / tol - 1.0) > 1e-6 and abs(h1[-2] / h1[0] / tol - 1.0) > 1e-6, case
            g = abs(true_residual_norm(entries_of(A), b, x1) - h1[-1]) / h1[-1]
            assert g < (1e-10 if tol == 1e-6 else 1e-6), (case, g)
        _, h0, _, _ = pcg(A, b, np.zeros_like(b), dinv, tol, 0)
        assert abs(h0[0] - h1[0]) > 1e-3 * h1[0], case  # x0 matters to the first residual
