"""Preconditioned CG, CPU side: the new entry points are exported by the product library, declared in api.h and listed; their
argument checks refuse bad calls before any HIP call (so they hold on a machine without a GPU); and the numpy restatement the
GPU tests compare against agrees with scipy's preconditioned CG, which pins the yardstick itself."""
import ctypes as C
import os
import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from conftest import ROOT
from pcg_restatement import diagonal, pcg, scaled_stencil5, stencil5

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
