"""Batched multigrid-preconditioned CG on the 3-D operator (csrc/multigrid3d_multi.hip), CPU side: both
libraries export the new creator and only the LAB build the stage hook; every refusal that include/spmv_amd/api.h and lab.h promise
before a HIP call holds on a machine without a GPU, with its sentence; and the one-column restatement
(tests/pcg_multi_multigrid3d_restatement.py) converges on the rows of multigrid3d_restatement.TABLE with n <= 33 in the table's own
iteration counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multigrid3d_restatement as M3
import pcg_multi_multigrid3d_restatement as MM3
import pcg_restatement as P
from conftest import ROOT

CREATOR = "spmv_amd_precond_create_multigrid3d_multi"
HOOK = "spmv_amd_mg_multi_stage3d"

# The rows of M3.TABLE with n <= 33. The restated column takes M3.TABLE's own count on every one of them: the batched dot shape
# (256-row partials, 4096-partial slices) moves the residuals in their last digits only, and a table row keeps its last two residuals
# at least M3.MARGIN = 15 % away from tol * ||r0||. So no count is moved and each is asserted as the table states it.
ROWS = [row for row in M3.TABLE if int(re.sub(r"\D", "", row[0])) <= 33]


def test_symbols_exported_declared_and_bound(B, Blab):
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    lab = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    exports = open(os.path.join(csrc, "exports.map")).read()
    exports_lab = open(os.path.join(csrc, "exports_lab.txt")).read()
    assert hasattr(B.lib(), CREATOR) and hasattr(Blab.lib(), CREATOR)
    assert re.search(r"\b" + CREATOR + r"\s*\(", api)
    assert re.search(r"^\s+" + CREATOR + r";", exports, flags=re.M)
    assert CREATOR in B.DECLARED_SYMBOLS and CREATOR not in B.LAB_ONLY_SYMBOLS
    assert getattr(B._pcg_lib(), CREATOR).argtypes is not None
    assert HOOK in B.LAB_ONLY_SYMBOLS and HOOK not in B.DECLARED_SYMBOLS
    assert not hasattr(B.lib(), HOOK) and hasattr(Blab.lib(), HOOK)
    assert re.search(r"\b" + HOOK + r"\s*\(", lab) and HOOK not in api
    assert re.search(r"^\s+" + HOOK + r";", exports_lab, flags=re.M) and HOOK not in exports
    assert getattr(Blab.lib(), HOOK).argtypes is not None
    assert callable(B.Precond.multigrid3d_multi) and callable(B.mg_multi_stage3d)
    for name in ("spmv_amd_mg3d_multi_level_product", "spmv_amd_precond_multigrid_level_spmm"):  # the level product's LAB-only knob and reader
        assert name in B.LAB_ONLY_SYMBOLS and not hasattr(B.lib(), name) and hasattr(Blab.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", lab) and name not in api and name not in exports, name
        assert re.search(r"^\s+" + name + r";", exports_lab, flags=re.M), name
    with pytest.raises(RuntimeError):
        B.mg3d_multi_level_product("csr")
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.mg_multi_stage3d("prolong3d", 1, B.MgMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_the_creator_refuses_without_touching_the_gpu(B, capfd):
    """spmv_amd_precond_create_multigrid3d's refusals in its order, max_rhs in front of them all."""
    _free_all(B)
    L = B._pcg_lib()
    bad = C.c_int(7)
    stencil7 = B.Operator("stencil7-csr").op

    def refused(op, nu, max_levels, max_rhs, word, bad_row=bad):
        bad.value = 7
        got = getattr(L, CREATOR)(op, nu, max_levels, max_rhs, None if bad_row is None else C.byref(bad_row))
        err = capfd.readouterr().err
        assert not got and (bad_row is None or bad.value == -1), (nu, max_levels, max_rhs)
        assert "[PCG]" in err and word in err, (nu, max_levels, max_rhs, word, err)

    refused(None, 1, 0, 4, "null operator")
    for nu in (-1, 9, -2 ** 31, 2 ** 31 - 1):
        refused(stencil7, nu, 0, 4, "smoother degree")
    for max_levels in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        refused(stencil7, 1, max_levels, 4, "max_levels")
    for max_rhs in (0, 9, -1, -2 ** 31, 2 ** 31 - 1):
        refused(stencil7, 1, 0, max_rhs, "max_rhs")
        refused(None, -1, 99, max_rhs, "max_rhs")  # in front of every other check
    refused(stencil7, -1, 99, 4, "smoother degree")  # then the 3-D creator's own order: nu before max_levels
    for mode in ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):  # not stencil7-csr: refused whether initialised or not
        refused(B.Operator(mode).op, 1, 0, 8, "is not stencil7-csr")
    for nu, max_levels, max_rhs in ((0, 0, 1), (1, 1, 3), (8, 32, 8)):  # stencil7-csr used before init
        refused(stencil7, nu, max_levels, max_rhs, "used before init")
    refused(stencil7, 1, 0, 8, "used before init", bad_row=None)  # bad_row may be NULL
    own = B.SpmvOperator()  # a caller's own table, even under the operator's name
    own.name = b"stencil7-csr"
    refused(C.pointer(own), 1, 0, 8, "is not stencil7-csr")
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d_multi(B.Operator("stencil7-csr"), 1, 0, 9)
    assert info.value.bad_row == -1
    with pytest.raises(ValueError) as info:
        B.Precond.multigrid3d_multi(B.Operator("stencil7-csr"), 1, 0, 0)
    assert info.value.bad_row == -1
    capfd.readouterr()


def test_the_stage_hook_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_mg_multi_stage3d (LAB build): an unknown stage, k outside 1..8, null arguments, a grid outside 2..674, a null or
    misaligned pointer the stage needs (a block vector: 16 bytes for even k, 8 bytes for odd k) -- each refused before any HIP call
    with a [PCG-MULTI] sentence. The pointers are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.MgMultiStageArgs(n=9, row_ptr=good, col_idx=good, values=good, z=good, r=good, coarse=good, d=good, dinv=good, c0=1.0, cols=None)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, k, a, word):
        rc = Blab.mg_multi_stage3d(stage, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG-MULTI]" in err and word in err and "refused" in err, (stage, k, word, rc, err)

    refused(None, 2, args(), "no stage named")
    for stage in ("smooth3d", "residual_restrict", "prolong", "term0", "term03d", "coarsen3d"):  # the 2-D names are the other hook's
        refused(stage, 2, args(), "unknown stage")
    for stage in ("stencil7_spmm", "spmm_csr"):  # a level's block product: the CSR, z in, d out
        for k in (0, 9, -1):
            refused(stage, k, args(), "k is not 1 to 8")
        refused(stage, 2, None, "null arguments")
        refused(stage, 2, args(n=675), "outside 2..674")
        for name in ("row_ptr", "col_idx", "values", "z", "d"):
            refused(stage, 2, args(**{name: None}), name + " is null")
        refused(stage, 2, args(d=odd), "d is not 16-byte aligned")
        refused(stage, 3, args(z=crooked), "z is not 8-byte aligned")
    for stage in ("residual_restrict3d", "prolong3d"):
        for k in (0, 9, -1):
            refused(stage, k, args(), "k is not 1 to 8")
        refused(stage, 2, None, "null arguments")
        for n in (1, 0, -5, 675, 46340):
            refused(stage, 2, args(n=n), "outside 2..674")
        refused(stage, 2, args(z=None), "z is null")
        refused(stage, 2, args(z=odd), "z is not 16-byte aligned")   # even k: 16-byte accesses
        refused(stage, 3, args(z=crooked), "z is not 8-byte aligned")  # odd k: 8-byte accesses, so `odd` itself would pass
        refused(stage, 4, args(cols=crooked), "cols is not 8-byte aligned")
        refused(stage, 2, args(coarse=None), "coarse is null")
        refused(stage, 4, args(coarse=odd), "coarse is not 16-byte aligned")
        refused(stage, 5, args(coarse=crooked), "coarse is not 8-byte aligned")
    for name in ("row_ptr", "col_idx", "values", "r"):
        refused("residual_restrict3d", 2, args(**{name: None}), name + " is null")
    refused("residual_restrict3d", 2, args(row_ptr=good + 2), "row_ptr is not 4-byte aligned")
    refused("residual_restrict3d", 2, args(col_idx=good + 2), "col_idx is not 4-byte aligned")
    refused("residual_restrict3d", 2, args(values=crooked), "values is not 8-byte aligned")
    refused("residual_restrict3d", 6, args(r=odd), "r is not 16-byte aligned")
    refused("residual_restrict3d", 7, args(r=crooked), "r is not 8-byte aligned")


def test_the_level_product_knob_refuses_an_unknown_word(Blab, capfd):
    for word in ("rowlds", "", "CSR", None):
        assert Blab.mg3d_multi_level_product(word) != 0
        err = capfd.readouterr().err
        assert "[PCG-MULTI]" in err and "auto, csr, stencil7" in err and "refused" in err
    assert Blab.mg3d_multi_level_product("auto") == 0
    assert Blab.lib().spmv_amd_precond_multigrid_level_spmm(None, 0) == b"none"


@pytest.mark.parametrize("row", ROWS, ids=[f"{r[0]}-nu{r[1]}-{r[2]:g}" for r in ROWS])
def test_the_restated_column_reproduces_the_table(row):
    name, nu, tol, table_count = row
    A, b, x0, n = M3.table_system(name)
    x, hist, its, converged, breakdown = MM3.solve(A, n, b, x0, nu, tol)
    print(f"{name} nu {nu} tol {tol}: {its} iterations (M3.TABLE: {table_count}), last two {hist[-2] / hist[0]:.4e} {hist[-1] / hist[0]:.4e}")
    assert converged and not breakdown and its == table_count and len(hist) == its + 1, (row, its)
    assert hist[-1] < tol * hist[0] <= hist[-2]
    assert P.true_residual_norm(P.entries_of(A), b, x) < tol * hist[0] * (1.0 + 1e-6)


def test_the_rows_are_the_ones_the_table_has_up_to_33():
    assert [r[0] for r in ROWS] == ["poisson16"] * 3 + ["poisson17", "poisson20"] + ["poisson32"] * 3 + ["poisson33"]
