"""Several right-hand sides per matrix pass, CPU side: the new entry points are exported by the product library and declared in
api.h, and their argument checks refuse bad calls before any HIP call -- so they hold on a machine without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ["spmv_amd_spmm_device", "spmv_amd_spmm_variant", "spmv_amd_block_to_device", "spmv_amd_block_to_host",
       "spmv_amd_cg_solve_device_multi", "spmv_amd_cg_last_history_multi", "spmv_amd_cg_multi_workspace_bytes"]


def test_multi_rhs_symbols_exported_declared_and_listed(B):
    L = B.lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS, name
        assert name not in B.LAB_ONLY_SYMBOLS


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory (nothing to release): safe without a GPU, and
    # it makes "used before init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack"):
        B.Operator(mode).free()


def test_spmm_argument_checks_refuse_without_touching_the_gpu(B):
    _free_all(B)
    L = B._multi_lib()
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    for k in (0, -1, 9, 100):
        assert L.spmv_amd_spmm_device(b"stencil5-csr", k, p, p) != 0
    assert L.spmv_amd_spmm_device(b"stencil5-csr", 2, None, p) != 0
    assert L.spmv_amd_spmm_device(b"stencil5-csr", 2, p, None) != 0
    assert L.spmv_amd_spmm_device(None, 2, p, p) != 0
    assert L.spmv_amd_spmm_device(b"no-such-operator", 2, p, p) != 0
    assert L.spmv_amd_spmm_device(b"ellpack", 2, p, p) != 0            # no multi-RHS path
    assert L.spmv_amd_spmm_device(b"stencil5-ellpack", 2, p, p) != 0
    assert L.spmv_amd_spmm_device(b"stencil5-csr", 2, p, p) != 0       # used before init
    assert L.spmv_amd_spmm_device(b"cusparse-csr", 1, p, p) != 0
    assert L.spmv_amd_spmm_device(b"stencil5-csr", 2, C.c_void_p(p.value + 4), p) != 0  # misaligned
    assert L.spmv_amd_spmm_variant(b"ellpack") == b"none"
    assert L.spmv_amd_spmm_variant(b"stencil5-csr") == b"uninitialised"
    assert L.spmv_amd_spmm_variant(b"nope") == b"unknown-operator"
    assert L.spmv_amd_block_to_device(0, 4, p, p) != 0 and L.spmv_amd_block_to_device(9, 4, p, p) != 0
    assert L.spmv_amd_block_to_host(2, 4, None, p) != 0 and L.spmv_amd_block_to_host(2, 4, p, None) != 0


def test_cg_multi_argument_checks_refuse_without_touching_the_gpu(B):
    _free_all(B)
    L = B._multi_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    Bk = np.ones((9, n))
    X = np.zeros((9, n))
    cfg = B.CGConfig(10, 1e-6, 0, 0)
    stats = (B.CGStats * 9)()

    def call(op, k, mat=m.ptr, b=Bk.ctypes.data, x=X.ctypes.data, c=C.byref(cfg), s=stats):
        return L.spmv_amd_cg_solve_device_multi(op, mat, k, b, x, c, s)

    stencil = B.Operator("stencil5-csr").op
    for k in (0, 9, -3):
        assert call(stencil, k) != 0
    assert call(stencil, 2, mat=None) != 0
    assert call(stencil, 2, b=None) != 0
    assert call(stencil, 2, x=None) != 0
    assert call(stencil, 2, c=None) != 0
    assert call(stencil, 2, s=None) != 0
    assert call(None, 2) != 0
    for mode in ("ellpack", "stencil5-ellpack"):
        assert call(B.Operator(mode).op, 2) != 0                         # no multi-RHS path
    assert call(stencil, 2) != 0                                         # used before init
    assert call(B.Operator("cusparse-csr").op, 1) != 0
    own = B.SpmvOperator()                                               # a caller's own vtable
    own.name = b"mine"
    assert call(C.pointer(own), 2) != 0
    with pytest.raises(RuntimeError):
        B.cg_solve_multi(B.Operator("stencil5-csr"), m, np.ones((2, n)), np.zeros((2, n)))
    # columns that no batched solve can have had; no workspace once the operators are freed
    assert L.spmv_amd_cg_last_history_multi(-1, None, 0) == -1
    assert L.spmv_amd_cg_last_history_multi(8, None, 0) == -1
    assert L.spmv_amd_cg_multi_workspace_bytes() == 0
