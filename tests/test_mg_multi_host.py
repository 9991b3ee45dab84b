"""Batched multigrid-preconditioned CG (csrc/multigrid_multi.hip), CPU side: both libraries export the new
entry points and only the LAB build its stage hook; every refusal that include/spmv_amd/api.h promises before a HIP call holds on a
machine without a GPU, with its sentence; and the one-column restatement (tests/pcg_multi_multigrid_restatement.py) converges on every
system of multigrid_restatement.TABLE with iteration counts pinned here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multigrid_restatement as MG
import pcg_multi_multigrid_restatement as MM
import pcg_restatement as P
from conftest import ROOT

NEW = ["spmv_amd_precond_create_multigrid_multi", "spmv_amd_precond_multigrid_max_rhs", "spmv_amd_precond_apply_device_multi"]
HOOK = "spmv_amd_mg_multi_stage"

# Iterations of the restatement's column on the rows of MG.TABLE, in its order, on the CPU. They are MG.TABLE's own counts on every
# row: the batched dot shape (256-row partials, 4096-partial slices) moves the residuals in their last digits only, and no row of
# the table has a residual that close to tol * ||r0|| (the nearest: poisson127 nu 1 tol 1e-6 stops at 0.9966e-6, scaled127 nu 1 tol
# 1e-10 passes 1.0098e-10 one iteration earlier).
COUNTS = [10, 17, 8, 17, 12, 20, 9, 12, 9, 6, 6, 5, 6, 10, 6, 10, 5, 9, 4, 9]


def test_symbols_exported_declared_and_bound(B, Blab):
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    lab = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    exports = open(os.path.join(csrc, "exports.map")).read()
    exports_lab = open(os.path.join(csrc, "exports_lab.txt")).read()
    for name in NEW:
        assert hasattr(B.lib(), name) and hasattr(Blab.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS and name not in B.LAB_ONLY_SYMBOLS, name
        assert getattr(B._pcg_lib(), name).argtypes is not None, name
    assert HOOK in B.LAB_ONLY_SYMBOLS and HOOK not in B.DECLARED_SYMBOLS
    assert not hasattr(B.lib(), HOOK) and hasattr(Blab.lib(), HOOK)
    assert re.search(r"\b" + HOOK + r"\s*\(", lab) and HOOK not in api
    assert re.search(r"^\s+" + HOOK + r";", exports_lab, flags=re.M) and HOOK not in exports
    for method in ("multigrid_multi", "multigrid_max_rhs", "apply_device_multi"):
        assert callable(getattr(B.Precond, method)), method
    assert callable(B.mg_multi_stage) and C.sizeof(B.MgMultiStageArgs) == 88
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.mg_multi_stage("term0", 1, B.MgMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_the_creator_refuses_without_touching_the_gpu(B, capfd):
    _free_all(B)
    L = B._pcg_lib()
    bad = C.c_int(7)
    stencil = B.Operator("stencil5-csr").op

    def refused(op, nu, max_levels, max_rhs, word, bad_row=bad):
        bad.value = 7
        got = L.spmv_amd_precond_create_multigrid_multi(op, nu, max_levels, max_rhs, None if bad_row is None else C.byref(bad_row))
        err = capfd.readouterr().err
        assert not got and (bad_row is None or bad.value == -1), (nu, max_levels, max_rhs)
        assert "[PCG]" in err and word in err, (nu, max_levels, max_rhs, word, err)

    refused(None, 1, 0, 4, "null operator")
    for nu in (-1, 9, -2 ** 31, 2 ** 31 - 1):
        refused(stencil, nu, 0, 4, "smoother degree")
    for max_levels in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        refused(stencil, 1, max_levels, 4, "max_levels")
    for max_rhs in (0, 9, -1, -2 ** 31, 2 ** 31 - 1):
        refused(stencil, 1, 0, max_rhs, "max_rhs")
        refused(None, 1, 0, max_rhs, "max_rhs")
    for mode in ("cusparse-csr", "ellpack", "stencil5-ellpack", "stencil7-csr"):  # not stencil5-csr: refused whether initialised or not
        refused(B.Operator(mode).op, 1, 0, 8, "is not stencil5-csr")
    for nu, max_levels, max_rhs in ((0, 0, 1), (1, 1, 3), (8, 32, 8)):  # stencil5-csr used before init
        refused(stencil, nu, max_levels, max_rhs, "used before init")
    refused(stencil, 1, 0, 8, "used before init", bad_row=None)  # bad_row may be NULL
    own = B.SpmvOperator()  # a caller's own table, even under the operator's name
    own.name = b"stencil5-csr"
    refused(C.pointer(own), 1, 0, 8, "is not stencil5-csr")
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid_multi(B.Operator("stencil5-csr"), 1, 0, 9)
    assert info.value.bad_row == -1
    capfd.readouterr()
    assert L.spmv_amd_precond_multigrid_max_rhs(None) == 0


def test_apply_multi_refuses_without_touching_the_gpu(B, capfd):
    """nrhs outside 1..8, a null argument, a misaligned block vector: refused before any HIP call, non-zero, with a [PCG-MULTI] sentence.
    The preconditioner handle is a block of zeros that these checks do not read beyond its size field (a real one needs a device: its
    refusals are in tests/test_mg_multi_gpu.py); the block vectors are addresses that are never dereferenced."""
    _free_all(B)
    L = B._pcg_lib()
    fake = (C.c_char * 4096)()
    handle = C.cast(fake, C.c_void_p)
    stencil = B.Operator("stencil5-csr").op
    good, other, odd = 4096, 1 << 20, 4096 + 8

    def refused(op, pc, k, r, z, word):
        rc = L.spmv_amd_precond_apply_device_multi(op, pc, k, r, z)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG-MULTI]" in err and word in err, (k, word, rc, err)

    for k in (0, 9, -3, 100, -2 ** 31, 2 ** 31 - 1):
        refused(stencil, handle, k, good, other, "right-hand sides")
        refused(None, None, k, None, None, "right-hand sides")
    refused(None, handle, 3, good, other, "null argument")
    refused(stencil, None, 3, good, other, "null argument")
    refused(stencil, handle, 3, None, other, "null argument")
    refused(stencil, handle, 3, good, None, "null argument")
    refused(stencil, handle, 2, odd, other, "16-byte aligned")
    refused(stencil, handle, 1, good, odd, "16-byte aligned")


def test_the_stage_hook_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_mg_multi_stage (LAB build): an unknown stage, k outside 1..8, null arguments, a grid out of range, a null or misaligned
    pointer the stage needs (a block vector: 16 bytes for even k, 8 bytes for odd k) -- each refused before any HIP call. The pointers
    are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.MgMultiStageArgs(n=9, row_ptr=good, col_idx=good, values=good, z=good, r=good, coarse=good, d=good, dinv=good, c0=1.0, cols=None)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, k, a, word):
        rc = Blab.mg_multi_stage(stage, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG-MULTI]" in err and word in err, (stage, k, word, rc, err)

    refused(None, 2, args(), "no stage named")
    refused("smooth", 2, args(), "unknown stage")
    refused("coarsen", 2, args(), "unknown stage")
    for stage in ("residual_restrict", "prolong", "term0"):
        for k in (0, 9, -1):
            refused(stage, k, args(), "k is not 1 to 8")
        refused(stage, 2, None, "null arguments")
        for n in (1, 0, -5, 46341):
            refused(stage, 2, args(n=n), "the fine grid is outside")
        refused(stage, 2, args(z=None), "z is null")
        refused(stage, 2, args(z=odd), "z is not 16-byte aligned")   # even k: 16-byte accesses
        refused(stage, 3, args(z=crooked), "z is not 8-byte aligned")  # odd k: 8-byte accesses, so `odd` itself would pass
        refused(stage, 4, args(cols=crooked), "cols is not 8-byte aligned")
    for name in ("row_ptr", "col_idx", "values", "r", "coarse"):
        refused("residual_restrict", 2, args(**{name: None}), name + " is null")
    refused("residual_restrict", 2, args(row_ptr=good + 2), "row_ptr is not 4-byte aligned")
    refused("residual_restrict", 2, args(values=crooked), "values is not 8-byte aligned")
    refused("residual_restrict", 6, args(r=odd), "r is not 16-byte aligned")
    refused("residual_restrict", 8, args(coarse=odd), "coarse is not 16-byte aligned")
    refused("residual_restrict", 5, args(coarse=crooked), "coarse is not 8-byte aligned")
    refused("prolong", 2, args(coarse=None), "coarse is null")
    refused("prolong", 4, args(coarse=odd), "coarse is not 16-byte aligned")
    for name in ("r", "d", "dinv"):
        refused("term0", 2, args(**{name: None}), name + " is null")
    refused("term0", 2, args(d=odd), "d is not 16-byte aligned")
    refused("term0", 7, args(r=crooked), "r is not 8-byte aligned")
    refused("term0", 2, args(dinv=crooked), "dinv is not 8-byte aligned")


@pytest.mark.parametrize("row, count", list(zip(MG.TABLE, COUNTS)), ids=[f"{r[0]}-nu{r[1]}-{r[2]:g}" for r in MG.TABLE])
def test_the_restated_column_converges_on_the_table(row, count):
    name, nu, tol, table_count = row
    A, b, x0, n = MG.table_system(name)
    x, hist, its, converged, breakdown = MM.solve(A, n, b, x0, nu, tol)
    print(f"{name} nu {nu} tol {tol}: {its} iterations (MG.TABLE: {table_count}), last two {hist[-2] / hist[0]:.4e} {hist[-1] / hist[0]:.4e}")
    assert converged and not breakdown and its == count and len(hist) == its + 1, (row, its)
    assert hist[-1] < tol * hist[0] <= hist[-2]
    assert P.true_residual_norm(P.entries_of(A), b, x) < tol * hist[0] * (1.0 + 1e-6)
