"""Batched BiCGSTAB, CPU side: the entry points are exported, declared and listed, the LAB build's stage hook is in the LAB build
only, every refusal that needs no device holds before any HIP call, and the INPUTS of the GPU tests are sound: on the table rows up
to grid127, rows127 and cube16 the restatement (tests/bicgstab_multi_restatement.py: the batched dot shape, the oracle's fma, the
operator's own product) takes the iteration count and the ending of the two CPU roundings and agrees with plain numpy within the
row's third-rounding bound; the seeded extra columns take the pinned counts and endings in every rounding and under both kinds; and
the 6 x 6 block-diagonal system ends each of its columns the way tests/test_bicgstab_multi_gpu.py asserts."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_multi_restatement as BM
from bicgstab_restatement import (TABLE, bicgstab, bicgstab_other_rounding, dinv_of, entries_of, hist_err, table_system,
                                  third_rounding_bound, true_residual_norm)
from conftest import ROOT

NEW = ["spmv_amd_bicgstab_solve_device_multi", "spmv_amd_bicgstab_last_history_multi", "spmv_amd_bicgstab_multi_workspace_bytes"]
HOOK = "spmv_amd_bicgstab_multi_stage"
ROWS = [i for i, r in enumerate(TABLE) if r[0] in ("grid33", "grid65", "grid127", "rows127", "cube16")]
IDS = [f"{TABLE[i][0]}-{TABLE[i][1]}-{TABLE[i][2]:g}" for i in ROWS]
STAGES = ("init", "dot_rv", "update_s", "dot_t", "update_xr", "direction")


def test_bicgstab_multi_symbols_exported_declared_and_listed(B, Blab):
    L = B.lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    lab = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    exports, exports_lab = open(os.path.join(csrc, "exports.map")).read(), open(os.path.join(csrc, "exports_lab.txt")).read()
    for name in NEW:
        assert hasattr(L, name) and hasattr(Blab.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS and name not in B.LAB_ONLY_SYMBOLS, name
    assert HOOK in B.LAB_ONLY_SYMBOLS and HOOK not in B.DECLARED_SYMBOLS
    assert hasattr(Blab.lib(), HOOK) and not hasattr(L, HOOK)
    assert re.search(r"\b" + HOOK + r"\s*\(", lab) and HOOK not in api
    assert re.search(r"^\s+" + HOOK + r";", exports_lab, flags=re.M) and HOOK not in exports
    for word in ("SpmvAmdBicgstabMultiColumn", "SpmvAmdBicgstabMultiStageArgs"):
        assert word in lab and word not in api
    col = B.BicgstabMultiColumn
    assert C.sizeof(col) == 96 and col.s_norm.offset == 56 and col.active.offset == 64 and col.x_step.offset == 84
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.bicgstab_multi_stage("reduce", "none", 1, B.BicgstabMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_bicgstab_multi_argument_checks_refuse_without_touching_the_gpu(B, capfd):
    """nrhs outside 1..8, a null argument, max_iters < 0, kinds "chebyshev" and "multigrid", an operator without a multi-RHS path, a
    caller's own table, an operator used before init: each refused before any HIP call, non-zero, with a [BICGSTAB-MULTI] sentence.
    The handle is a record of zeros (kind "none") that no later check reaches; a real one needs a device (its refusals:
    tests/test_bicgstab_multi_gpu.py)."""
    _free_all(B)
    L = B._bicgstab_multi_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    Bk, X = np.ones((9, n)), np.zeros((9, n))
    cfg = B.CGConfig(10, 1e-6, 0, 0)
    stats = (B.CGStats * 9)()
    record = (C.c_int * 1024)()
    handle = C.cast(record, C.c_void_p)

    def refused(op, k, mat=m.ptr, pc=handle, b=Bk.ctypes.data, x=X.ctypes.data, c=C.byref(cfg), s=stats, word=""):
        rc = L.spmv_amd_bicgstab_solve_device_multi(op, mat, pc, k, b, x, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and "[BICGSTAB-MULTI]" in err and word in err, (k, word, rc, err)

    stencil = B.Operator("stencil5-csr").op
    for k in (0, 9, -3, 100):
        refused(stencil, k, word="right-hand sides")
    refused(stencil, 2, mat=None, word="null argument")
    refused(stencil, 2, pc=None, word="null argument")
    refused(stencil, 2, b=None, word="null argument")
    refused(stencil, 2, x=None, word="null argument")
    refused(stencil, 2, c=None, word="null argument")
    refused(stencil, 2, s=None, word="null argument")
    refused(None, 2, word="null argument")
    refused(stencil, 2, c=C.byref(B.CGConfig(-1, 1e-6, 0, 0)), word="max_iters < 0")
    for mode in ("ellpack", "stencil5-ellpack"):
        refused(B.Operator(mode).op, 2, word="no multi-RHS path")
    own = B.SpmvOperator()  # a caller's own vtable
    own.name = b"mine"
    refused(C.pointer(own), 2, word="no multi-RHS path")
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr"):
        refused(B.Operator(mode).op, 1, word="used before init")
    # the first two ints of SpmvAmdPrecond are kind and n (csrc/precond.hpp); kinds 2 and 3 are "chebyshev" and "multigrid"
    for kind, word in ((2, "chebyshev"), (3, "multigrid")):
        record[0], record[1] = kind, n
        refused(stencil, 2, word=word)
        refused(stencil, 2, word="symmetric definite")
    assert np.all(X == 0.0)
    assert L.spmv_amd_bicgstab_last_history_multi(-1, None, 0) == -1
    assert L.spmv_amd_bicgstab_last_history_multi(8, None, 0) == -1
    assert B.bicgstab_multi_workspace_bytes() == 0


def test_bicgstab_multi_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_bicgstab_multi_stage (LAB build): an unknown stage or kind, k outside 1..8, null arguments, a null or misaligned
    pointer the stage needs, n < 1, count < 1, which outside 0..4, hist_cap < 0 -- each refused before any HIP call. The pointers are
    never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.BicgstabMultiStageArgs(n=5, X=good, R=good, RH=good, P=good, PH=good, SH=good, V=good, T=good, dinv=good, cols=good,
                                        partials=good, count=3, which=4, tol=1e-6, hist=good, hist_cap=4)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, kind, k, a, word):
        rc = Blab.bicgstab_multi_stage(stage, kind, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[BICGSTAB-MULTI]" in err and "refused" in err and word in err, (stage, kind, k, word, rc, err)

    for stage in (None, "", "Init", "update", "update_r", "update_xp", "spmm"):
        refused(stage, "jacobi", 2, args(), "stage")
    for stage in STAGES + ("reduce",):
        for k in (0, -1, 9, 100):
            refused(stage, "jacobi", k, args(), "k is not 1 to 8")
        refused(stage, "jacobi", 2, None, "null arguments")
    # the block vectors a stage needs under kind "jacobi"; under "none" dinv, PH and SH are not looked at (update_xr reads P instead)
    needs = {"init": ("V", "R", "RH", "P", "PH"), "dot_rv": ("RH", "V"), "update_s": ("V", "R", "SH"), "dot_t": ("T", "R"),
             "update_xr": ("X", "R", "T", "RH", "PH", "SH"), "direction": ("P", "V", "R", "PH")}
    for stage, vectors in needs.items():
        if stage not in ("dot_rv", "dot_t"):
            for kind in (None, "", "ilu0", "Jacobi", "chebyshev", "multigrid"):
                refused(stage, kind, 2, args(), "kind")
        refused(stage, "jacobi", 2, args(n=0), "n < 1")
        for k in (1, 2, 5, 8):
            for name in vectors:
                for kind in ("jacobi", "none"):
                    if kind == "none" and name in ("PH", "SH"):
                        continue  # not looked at
                    refused(stage, kind, k, args(**{name: None}), name + " is null")
                    refused(stage, kind, k, args(**{name: odd}), name + " is not 16-byte aligned")
        if stage in ("init", "update_s", "direction"):
            refused(stage, "jacobi", 2, args(dinv=None), "dinv is null")
            refused(stage, "jacobi", 2, args(dinv=crooked), "dinv is not 8-byte aligned")
        if stage == "update_xr":
            refused(stage, "none", 2, args(P=None), "P is null")
        if stage != "direction":
            refused(stage, "none", 2, args(partials=None), "partials is null")
            refused(stage, "none", 2, args(partials=crooked), "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, "none", 2, args(cols=None), "cols is null")
            refused(stage, "none", 2, args(cols=crooked), "cols is not 8-byte aligned")
    for count in (0, -1):
        refused("reduce", None, 2, args(count=count), "count < 1")
    for which in (-1, 5):
        refused("reduce", None, 2, args(which=which), "which")
    refused("reduce", None, 2, args(hist_cap=-1), "hist_cap < 0")
    refused("reduce", None, 2, args(partials=None), "partials is null")
    refused("reduce", None, 2, args(partials=crooked), "partials is not 8-byte aligned")
    refused("reduce", None, 2, args(cols=None), "cols is null")
    refused("reduce", None, 2, args(hist=None), "hist is null")
    refused("reduce", None, 2, args(hist=crooked), "hist is not 8-byte aligned")


# ---------------------------------------------------------------- the systems of the whole-solve tests
def products_of(O, name):
    """The products the GPU tests' operators make of a table system: name -> matvec."""
    A, _, _ = table_system(name)
    rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
    out = {"csr": lambda u: O.spmv_csr(rp, ci, va, u)}
    if not name.startswith("cube"):
        grid = int(round(np.sqrt(A.shape[0])))
        out["stencil5"] = lambda u: O.spmv_stencil5(rp, ci, va, u, grid)
    return out


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_the_restatement_holds_the_table(O, row):
    """Column 0 of every whole-solve batch. The batched dot shape is one more rounding of the same algebra: the table's count and
    ending in the exact form (on every product the GPU tests use) and with the dot shape alone in plain numpy, history and x within
    third_rounding_bound(stored) of bicgstab(), the true residual below 1.01 tol ||r0||."""
    name, kind, tol, iterations, end, stored = TABLE[row]
    bound = third_rounding_bound(stored)
    A, b, x0 = table_system(name)
    d = dinv_of(A, kind)
    x1, h1, i1, c1, e1 = bicgstab(A, b, x0, d, tol)
    _, _, i2, c2, e2 = bicgstab_other_rounding(A, b, x0, d, tol)
    assert i1 == i2 == iterations and c1 and c2 and e1 == e2 == end
    runs = {"numpy": BM.solve_numpy(A, b, x0, d, tol)}
    for family, matvec in products_of(O, name).items():
        runs[family] = BM.solve(matvec, b, x0, d, tol)
    for what, (x, h, it, conv, how) in runs.items():
        err = hist_err(h, h1)
        print(f"{(name, kind, tol)} {what}: {it} iterations, ends by the {how} step, against plain numpy {err:.2e} (bound {bound:.0e})")
        assert it == iterations and conv and how == end, (what, it, how)
        assert len(h) == iterations + 1 and err <= bound, (what, err)
        assert np.max(np.abs(x - x1)) <= bound * np.max(np.abs(x1)), what
        assert true_residual_norm(entries_of(A), b, x) <= 1.01 * tol * h[0], what


@pytest.mark.parametrize("name", sorted(BM.SEEDED))
def test_the_seeded_columns_take_the_pinned_counts_in_every_rounding(O, name):
    """Columns 1..8: the exact form on every product, the dot shape alone, plain numpy and the long-double rounding take the pinned
    count and end the pinned way under both kinds -- so no rounding of a sum decides when a column stops -- and the columns stop in
    different iterations, by the half step and by the whole one: the whole-solve tests exercise freezing."""
    A, _, _ = table_system(name)
    products = products_of(O, name)
    for s, (iterations, end) in enumerate(BM.SEEDED[name], start=1):
        b, x0 = BM.seeded_column(name, s)
        for kind in ("none", "jacobi"):
            d = dinv_of(A, kind)
            runs = [bicgstab(A, b, x0, d, BM.TOL), bicgstab_other_rounding(A, b, x0, d, BM.TOL), BM.solve_numpy(A, b, x0, d)]
            runs += [BM.solve(matvec, b, x0, d) for matvec in products.values()]
            assert all((r[2], r[3], r[4]) == (iterations, True, end) for r in runs), (name, s, kind, [r[2:] for r in runs])
            err = max(hist_err(r[1], runs[0][1]) for r in runs[1:])
            print(f"{name} column {s} {kind}: {iterations} iterations, {end} step, the roundings disagree by {err:.2e}")
            assert err <= 1e-6, (name, s, kind, err)
    counts = [c for c, _ in BM.SEEDED[name]]
    assert len(set(counts)) >= 5 and {e for _, e in BM.SEEDED[name]} == {"half", "whole"}


def test_batches_are_the_table_system_and_the_seeded_columns():
    Bk, X0 = BM.batch("grid33", 3)
    _, b, x0 = table_system("grid33")
    rng = np.random.default_rng(1002)
    assert Bk.shape == X0.shape == (3, 33 * 33) and np.array_equal(Bk[0], b) and np.array_equal(X0[0], x0)
    assert np.array_equal(Bk[2], rng.standard_normal(33 * 33)) and np.array_equal(X0[2], rng.standard_normal(33 * 33))


# ---------------------------------------------------------------- every end in one batch
BLOCKS = sp.block_diag([np.array([[0.0, 1.0], [1.0, 0.0]]), 3.0 * np.eye(2), 2.0 * np.eye(2)]).tocsr()
BLOCK_B = np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.5, -0.75, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.5, -0.75]])
BLOCK_ENDS = {1e-6: ["sigma", "half", "half"], 0.0: ["sigma", "max_iters", "omega"]}
BLOCK_CAP = 4


def test_every_end_in_one_batch_on_the_cpu(O):
    """The three 2 x 2 systems of tests/test_bicgstab_gpu.py as the blocks of one 6 x 6 matrix, one column supported on each block.
    [[0, 1], [1, 0]]: sigma = 0 in iteration 1. 3 I: alpha = fl(1 / 3), so s = fma(-alpha, 3 b, b) is tiny but not 0 -- the half
    step at tol 1e-6, an ordinary iteration (it goes on to the cap) at tol 0. 2 I: alpha = 0.5 exactly, s = 0 -- the half step at
    tol 1e-6, the omega breakdown (t.t = 0) at tol 0."""
    rp, ci, va = O.build_csr(entries_of(BLOCKS), 6)
    for tol, ends in BLOCK_ENDS.items():
        for j, end in enumerate(ends):
            x, h, it, conv, how = BM.solve(lambda u: O.spmv_csr(rp, ci, va, u), BLOCK_B[j], np.zeros(6), None, tol, BLOCK_CAP)
            assert how == end and conv == (end == "half") and it == (BLOCK_CAP if end == "max_iters" else 1), (tol, j, how, it)
            assert np.all(np.isfinite(x))
            if end == "sigma":
                assert np.array_equal(x, np.zeros(6)) and np.array_equal(h, [1.0, 1.0])
            else:
                want = BLOCK_B[j] / (3.0 if j == 1 else 2.0)
                assert np.max(np.abs(x - want)) <= 1e-15 and h[1] < 1e-15 * h[0]
