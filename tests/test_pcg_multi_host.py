"""Batched preconditioned CG, CPU side: the entry points are exported, declared and listed, the LAB build's stage hook is in the LAB
build only, every refusal that needs no device holds before any HIP call, the batched dot of tests/pcg_multi_restatement.py is held
against math.fsum, and the systems of the whole-solve tests (tests/test_pcg_multi_gpu.py) are shown to be honest ones: with the
batched dot shape they take exactly the iteration counts of chebyshev_restatement.TABLE, their histories agree with pcg() to 1e-12
and their last two residuals stay 5 % clear of tol * ||r0||, so no rounding of a sum decides an iteration count."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import chebyshev_restatement as CH
import pcg_multi_restatement as PM
import pcg_restatement as P
from conftest import ROOT

SUM_TOL = 1e-13  # a re-ordered fp64 sum against math.fsum, of sum|terms| (tests/test_multi_rhs_host.py)
HIST_TOL = 1e-12
MARGIN = 0.05

NEW = ["spmv_amd_pcg_solve_device_multi", "spmv_amd_pcg_last_history_multi", "spmv_amd_pcg_multi_workspace_bytes"]
HOOK = "spmv_amd_pcg_multi_stage"

# (system, degree or None = Jacobi): the rows of chebyshev_restatement.TABLE the GPU tests solve, all at tol 1e-6
ROWS = [("scaled127", None), ("negated65", None), ("plain127", None), ("plain601", None), ("scaled601", None),
        ("poisson127", 4), ("poisson127", 8), ("plain127", 2), ("scaled127", 4), ("negated65", 8), ("scaled601", 2)]
COUNTS = [18, 18, 19, 19, 18, 69, 45, 13, 8, 5, 13]


def test_pcg_multi_symbols_exported_declared_and_listed(B):
    L = B.lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS, name
        assert name not in B.LAB_ONLY_SYMBOLS


def test_the_stage_hook_is_a_lab_symbol_only(B, Blab):
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    assert HOOK in B.LAB_ONLY_SYMBOLS and HOOK not in B.DECLARED_SYMBOLS
    assert not hasattr(B.lib(), HOOK) and hasattr(Blab.lib(), HOOK)
    assert HOOK not in open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    assert re.search(r"\b" + HOOK + r"\s*\(", open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read())
    assert HOOK not in open(os.path.join(csrc, "exports.map")).read()
    assert re.search(r"^\s+" + HOOK + r";", open(os.path.join(csrc, "exports_lab.txt")).read(), flags=re.M)
    assert C.sizeof(B.PcgMultiColumn) == 80 and B.PcgMultiColumn.active.offset == 48 and B.PcgMultiColumn.skip_update.offset == 68
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.pcg_multi_stage("reduce", "none", 1, B.PcgMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack"):
        B.Operator(mode).free()


def test_pcg_multi_argument_checks_refuse_without_touching_the_gpu(B, capfd):
    """nrhs outside 1..8, a null argument, max_iters < 0, an operator without a multi-RHS path, a caller's own table, an operator
    used before init: each refused before any HIP call, non-zero, with a [PCG-MULTI] sentence. The preconditioner handle here is a
    block of zeros that no check reaches (a real one needs a device; its refusals are in tests/test_pcg_multi_gpu.py)."""
    _free_all(B)
    L = B._pcg_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    Bk = np.ones((9, n))
    X = np.zeros((9, n))
    cfg = B.CGConfig(10, 1e-6, 0, 0)
    stats = (B.CGStats * 9)()
    fake = (C.c_char * 4096)()
    handle = C.cast(fake, C.c_void_p)

    def refused(op, k, mat=m.ptr, pc=handle, b=Bk.ctypes.data, x=X.ctypes.data, c=C.byref(cfg), s=stats, word=""):
        rc = L.spmv_amd_pcg_solve_device_multi(op, mat, pc, k, b, x, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG-MULTI]" in err and word in err, (k, word, rc, err)

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
    assert L.spmv_amd_pcg_last_history_multi(-1, None, 0) == -1
    assert L.spmv_amd_pcg_last_history_multi(8, None, 0) == -1
    assert L.spmv_amd_pcg_multi_workspace_bytes() == 0


def test_pcg_multi_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_pcg_multi_stage (LAB build): an unknown stage or kind, cheb_step with another kind, k outside 1..8, null arguments, a
    null or misaligned pointer the stage needs, n < 1, count < 1, which outside 0..4, hist_cap < 0 -- each refused before any HIP
    call. The pointers are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.PcgMultiStageArgs(n=5, X=good, R=good, P=good, AP=good, D=good, Z=good, dinv=good, cols=good, partials=good, count=3, which=2,
                                   tol=1e-6, hist=good, hist_cap=4, c0=1.0, g=1.0, h=0.5, last=1)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, kind, k, a, word):
        rc = Blab.pcg_multi_stage(stage, kind, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[PCG-MULTI]" in err and "refused" in err and word in err, (stage, kind, k, word, rc, err)

    for stage in (None, "", "Init", "update", "step", "spmm"):
        refused(stage, "jacobi", 2, args(), "stage")
    vector_stages = ("init", "update_r", "update_xp", "cheb_step")
    for stage in vector_stages + ("reduce",):
        for k in (0, -1, 9, 100):
            refused(stage, "chebyshev", k, args(), "k is not 1 to 8")
        refused(stage, "chebyshev", 2, None, "null arguments")
    for stage in vector_stages:
        for kind in (None, "", "multigrid", "Jacobi"):
            refused(stage, kind, 2, args(), "kind")
        refused(stage, "chebyshev", 2, args(n=0), "n < 1")
        refused(stage, "chebyshev", 2, args(dinv=None), "dinv is null")
        refused(stage, "chebyshev", 2, args(dinv=crooked), "dinv is not 8-byte aligned")
    for kind in ("none", "jacobi"):
        refused("cheb_step", kind, 2, args(), "belongs to kind chebyshev")
    needs = {("init", "none"): ("AP", "R", "P"), ("init", "chebyshev"): ("AP", "R", "D", "Z"), ("update_r", "jacobi"): ("AP", "R"),
             ("update_r", "chebyshev"): ("AP", "R", "D", "Z"), ("cheb_step", "chebyshev"): ("AP", "R", "D", "Z"),
             ("update_xp", "jacobi"): ("R", "P", "X"), ("update_xp", "chebyshev"): ("Z", "P", "X")}
    for (stage, kind), vectors in needs.items():
        for k in (1, 2, 5, 8):
            for name in vectors:
                refused(stage, kind, k, args(**{name: None}), name + " is null")
                refused(stage, kind, k, args(**{name: odd}), name + " is not 16-byte aligned")
        if stage != "update_xp":
            refused(stage, kind, 2, args(partials=None), "partials is null")
            refused(stage, kind, 2, args(partials=crooked), "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, kind, 2, args(cols=None), "cols is null")
            refused(stage, kind, 2, args(cols=crooked), "cols is not 8-byte aligned")
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


# ---------------------------------------------------------------- the batched dot
@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257, 1000, 4097, 300000, 1100000])
def test_batched_dot_against_fsum(rows):
    """300000 rows: 1172 partials, one slice; 1100000: 4297 partials, a second, short slice."""
    rng = np.random.default_rng(rows)
    u, v = rng.standard_normal(rows), rng.standard_normal(rows)
    terms = u * v
    got = PM.dot(u, v)
    assert abs(got - math.fsum(terms)) <= SUM_TOL * math.fsum(np.abs(terms))
    assert PM.dot(v, u) == got  # the rounded product commutes: the same bits


# ---------------------------------------------------------------- the systems of the whole-solve tests
def test_the_rows_are_rows_of_the_table():
    table = {(name, degree): its for name, degree, tol, its in CH.TABLE if tol == 1e-6}
    assert [table[row] for row in ROWS] == COUNTS


@pytest.mark.parametrize("row, want", list(zip(ROWS, COUNTS)), ids=[f"{n}-{'jacobi' if d is None else d}" for n, d in ROWS])
def test_whole_solve_systems_are_honest(row, want):
    name, degree = row
    tol = 1e-6
    A, b, x0 = CH.table_system(name)
    dinv = 1.0 / P.diagonal(A)
    if degree is None:
        coef = None
        _, ref, ref_its, ref_ok = P.pcg(A, b, x0, dinv, tol=tol)
    else:
        lo, hi = CH.interval(A, dinv)
        coef = CH.coefficients(degree, lo, hi)
        _, ref, ref_its, ref_ok = CH.pcg(A, b, x0, degree, lo, hi, tol=tol)
    _, hist, its, ok = PM.solve_numpy(A, b, x0, dinv, coef, tol=tol)
    assert its == ref_its == want and ok and ref_ok
    err = P.hist_err(hist, ref)
    bound = tol * hist[0]
    margin = min(hist[-2] / bound - 1.0, 1.0 - hist[-1] / bound)
    print(f"{name} degree {degree}: {its} iterations, history difference {err:.1e}, margin {100 * margin:.1f} %")
    assert err <= HIST_TOL
    assert margin >= MARGIN
