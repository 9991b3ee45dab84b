"""BiCGSTAB, CPU side: the new entry points are exported, declared and listed; the argument checks of the solve and of the LAB
build's spmv_amd_bicgstab_stage refuse bad calls before any HIP call (so they hold on a machine without a GPU); and the INPUTS of
the GPU tests are sound: on every row of bicgstab_restatement.TABLE two roundings of the restatement take the recorded iteration
count, end the recorded way and agree within the recorded bound, the bit-exact form agrees with them within it, and every converged
row's true residual in long double is below the tolerance."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from bicgstab_restatement import (APP_CASE, TABLE, bicgstab, bicgstab_exact, bicgstab_other_rounding, convdiff5, convdiff7, dinv_of, entries_of,
                                  hist_err, table_system, third_rounding_bound, true_residual_norm)
from conftest import ROOT

NEW = ["spmv_amd_bicgstab_solve_device", "spmv_amd_bicgstab_last_history"]
HOOK = "spmv_amd_bicgstab_stage"
IDS = [f"{r[0]}-{r[1]}-{r[2]:g}" for r in TABLE]


def test_bicgstab_symbols_exported_declared_and_listed(B, Blab):
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


def test_the_matrices_are_what_the_issue_says():
    """convdiff5: centre 4 + px + py + shift, W = -1 - px, N = -1 - py, E = S = -1 (row i = grid row * n + column); |A - A^T|
    reaches px. The 3-D twin the same with D = -1 - pz. Row scaling multiplies ROWS."""
    n = 5
    A = convdiff5(n, 2.0, 0.5, 0.25).toarray()
    i = 2 * n + 2
    assert A[i, i] == 6.75 and A[i, i - 1] == -3.0 and A[i, i + 1] == -1.0 and A[i, i - n] == -1.5 and A[i, i + n] == -1.0
    assert np.count_nonzero(A[i]) == 5 and np.max(np.abs(A - A.T)) == 2.0
    assert A[n, n - 1] == 0.0 and A[n - 1, n] == 0.0  # no wrap between grid rows
    A3 = convdiff7(4, 2.0, 0.5, 1.0, 0.5).toarray()
    j = 16 + 4 + 1
    assert A3[j, j] == 10.0 and A3[j, j - 1] == -3.0 and A3[j, j - 4] == -1.5 and A3[j, j - 16] == -2.0
    assert A3[j, j + 1] == A3[j, j + 4] == A3[j, j + 16] == -1.0 and np.count_nonzero(A3[j]) == 7
    S = convdiff5(n, decades=2.0, seed=3).toarray()
    scale = S[np.arange(n * n), np.arange(n * n)] / 7.0
    assert np.all(scale >= 1.0) and np.all(scale < 100.0) and np.ptp(scale) > 10.0
    assert np.allclose(S, scale[:, None] * convdiff5(n).toarray(), rtol=1e-15)


@functools.lru_cache(maxsize=None)
def _two_roundings(row):
    name, kind, tol, _, _, _ = TABLE[row]
    A, b, x0 = table_system(name)
    d = dinv_of(A, kind)
    return bicgstab(A, b, x0, d, tol), bicgstab_other_rounding(A, b, x0, d, tol)


@pytest.mark.parametrize("row", range(len(TABLE)), ids=IDS)
def test_the_table_holds_in_two_roundings(row):
    """Equal iteration counts -- the table's --, the same ending (half step or whole step), histories within the stored bound, the
    converging ratio not a rounding error away from tol, and the true residual of a converged row <= 1.01 tol ||r0||."""
    name, kind, tol, iterations, end, bound = TABLE[row]
    A, b, x0 = table_system(name)
    (x1, h1, i1, c1, e1), (x2, h2, i2, c2, e2) = _two_roundings(row)
    case = (name, kind, tol)
    assert i1 == i2 == iterations and c1 and c2 and e1 == e2 == end, (case, i1, i2, e1, e2)
    err = hist_err(h1, h2)
    print(f"{case}: {i1} iterations, ends by the {e1} step, the roundings disagree by {err:.2e} (bound {bound:.0e})")
    assert len(h1) == len(h2) == iterations + 1 and err <= bound, (case, err)
    assert h1[-1] / h1[0] < tol <= h1[-2] / h1[0]
    assert abs(h1[-1] / h1[0] / tol - 1.0) > 1e3 * bound, case
    e = entries_of(A)
    for x, h in ((x1, h1), (x2, h2)):
        assert true_residual_norm(e, b, x) <= 1.01 * tol * h[0], case
    _, h0, _, _, _ = bicgstab(A, b, np.zeros_like(b), dinv_of(A, kind), tol, 0)
    assert abs(h0[0] - h1[0]) > 1e-3 * h1[0], case  # x0 matters to the first residual


@pytest.mark.parametrize("row", range(len(TABLE)), ids=IDS)
def test_the_exact_form_agrees_with_plain_numpy(O, row):
    """bicgstab_exact -- the product in the operator's bits, the dots as the kernels sum them, every update an fma -- is a third
    rounding of the same algebra: the table's count and ending, history and x within the row's bound for a third rounding,
    max(1e-10, 10 x the stored disagreement) -- what the device, which equals this form bit for bit, is held to against plain numpy."""
    name, kind, tol, iterations, end, stored = TABLE[row]
    bound = third_rounding_bound(stored)
    A, b, x0 = table_system(name)
    (x1, h1, _, _, _), _ = _two_roundings(row)
    rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
    grid = int(round(np.sqrt(A.shape[0])))
    matvec = (lambda u: O.spmv_csr(rp, ci, va, u)) if name.startswith("cube") else (lambda u: O.spmv_stencil5(rp, ci, va, u, grid))
    x, h, it, conv, how = bicgstab_exact(matvec, b, x0, dinv_of(A, kind), tol)
    err = hist_err(h, h1)
    print(f"{(name, kind, tol)}: exact against plain {err:.2e} (bound {bound:.0e})")
    assert it == iterations and conv and how == end and err <= bound
    assert np.max(np.abs(x - x1)) <= bound * np.max(np.abs(x1))
    assert true_residual_norm(entries_of(A), b, x) <= 1.01 * tol * h[0]


def test_the_application_case_holds_in_every_rounding(O):
    """b = 1, x0 = 0 on the 33 grid (what apps/cg_solver solves on the written file): APP_CASE's count for both kinds in the two
    CPU roundings and in the exact form on both products, and the converging ratio far from tol."""
    n, iterations = APP_CASE
    A = convdiff5(n)
    b, x0 = np.ones(n * n), np.zeros(n * n)
    rp, ci, va = O.build_csr(entries_of(A), n * n)
    for kind in ("none", "jacobi"):
        d = dinv_of(A, kind)
        runs = [bicgstab(A, b, x0, d), bicgstab_other_rounding(A, b, x0, d),
                bicgstab_exact(lambda u: O.spmv_csr(rp, ci, va, u), b, x0, d),
                bicgstab_exact(lambda u: O.spmv_stencil5(rp, ci, va, u, n), b, x0, d)]
        assert all(r[2] == iterations and r[3] for r in runs), (kind, [r[2:] for r in runs])
        h = runs[0][1]
        assert h[-1] / h[0] < 0.5e-6 and h[-2] / h[0] > 1.4e-6


def test_breakdowns_and_the_half_step_in_the_restatement(O):
    """The three 2 x 2 systems of the GPU test, in plain numpy: sigma = 0 stops iteration 1 with x untouched and the unchanged
    residual recorded; A = 3 I converges by the half step with x = b / 3 and no omega; at tol 0 the same system is an omega
    breakdown (t.t = 0) that keeps the half step's x and records ||s|| = 0."""
    import scipy.sparse as sp

    swap = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    x, h, it, conv, end = bicgstab(swap, np.array([1.0, 0.0]), np.zeros(2), None)
    assert (it, conv, end) == (1, False, "sigma") and np.array_equal(x, [0.0, 0.0]) and np.array_equal(h, [1.0, 1.0])
    three = sp.csr_matrix(3.0 * np.eye(2))
    b = np.array([1.5, -0.75])
    x, h, it, conv, end = bicgstab(three, b, np.zeros(2), None, 1e-6)
    assert (it, conv, end) == (1, True, "half") and np.array_equal(x, b / 3.0) and h[1] == 0.0
    x, h, it, conv, end = bicgstab(three, b, np.zeros(2), None, 0.0)
    assert (it, conv, end) == (1, False, "omega") and np.array_equal(x, b / 3.0) and h[1] == 0.0 and len(h) == 2
    # with the fma the device's algebra prescribes, s = fma(-fl(1/3), 3 b, b) = b * 2^-54 is NOT zero: on 3 I the exact form takes the
    # half step at tol 1e-6 with a tiny recorded residual and, at tol 0, goes on (no omega breakdown); on 2 I alpha = 0.5 is exact
    # and the omega breakdown is there in every rounding (tests/test_bicgstab_gpu.py solves these on the device)
    for scale, tol, want_end, want_it in ((3.0, 1e-6, "half", 1), (3.0, 0.0, "max_iters", 4), (2.0, 0.0, "omega", 1)):
        rp, ci, va = O.build_csr(entries_of(sp.csr_matrix(scale * np.eye(2))), 2)
        x, h, it, conv, end = bicgstab_exact(lambda u: O.spmv_csr(rp, ci, va, u), b, np.zeros(2), None, tol, 4)
        assert (end, it) == (want_end, want_it) and np.max(np.abs(x - b / scale)) <= 1e-16, (scale, tol, end, it)
        if scale == 3.0:
            assert 0.0 < h[1] < 1e-15
        else:
            assert h[1] == 0.0 and np.array_equal(x, b / 2.0) and not conv


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_bicgstab_solve_refuses_without_touching_the_gpu(B, capfd):
    _free_all(B)
    L = B._pcg_lib()
    L.spmv_amd_bicgstab_solve_device.argtypes = L.spmv_amd_pcg_solve_device.argtypes
    L.spmv_amd_bicgstab_last_history.argtypes = [C.c_void_p, C.c_int]
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    b, x = np.ones(n), np.zeros(n)
    cfg, st = B.CGConfig(10, 1e-6, 0, 0), B.CGStats()
    fake = C.c_void_p(16)  # never dereferenced: every call it is given to is refused before the preconditioner is looked at

    def refused(op, pm=None, mat=m.ptr, bb=b.ctypes.data, xx=x.ctypes.data, c=C.byref(cfg), s=C.byref(st), word="[BICGSTAB]"):
        rc = L.spmv_amd_bicgstab_solve_device(op, mat, pm, bb, xx, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and "[BICGSTAB]" in err and word in err and err.count("\n") == 1, (rc, err)

    stencil = B.Operator("stencil5-csr").op
    refused(stencil, word="null argument")                 # no preconditioner
    refused(None, fake, word="null argument")
    refused(stencil, fake, mat=None, word="null argument")
    refused(stencil, fake, bb=None, word="null argument")
    refused(stencil, fake, xx=None, word="null argument")
    refused(stencil, fake, c=None, word="null argument")
    refused(stencil, fake, s=None, word="null argument")
    own = B.SpmvOperator()                                  # a caller's vtable without run_device
    own.name = b"mine"
    refused(C.pointer(own), fake, word="device-native")
    neg = B.CGConfig(-1, 1e-6, 0, 0)
    refused(stencil, fake, c=C.byref(neg), word="max_iters")
    assert np.all(x == 0.0)
    assert L.spmv_amd_bicgstab_last_history(None, 0) >= 0
    L.spmv_amd_pcg_release_workspace()                      # nothing held: a no-op


def test_bicgstab_solve_refuses_what_needs_a_real_preconditioner_record(B, capfd):
    """With a record made without a GPU (kind "none" on a caller's diagonal is not offered, so: spmv_amd_precond_create refuses
    an uninitialised operator) the remaining refusals cannot be reached on the CPU through the creators; they are reached with
    the operator check that comes first: every operator of the library used before init is refused before the pair is looked at --
    after the kind, which is read from the record."""
    _free_all(B)
    L = B._pcg_lib()
    L.spmv_amd_bicgstab_solve_device.argtypes = L.spmv_amd_pcg_solve_device.argtypes
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    b, x = np.ones(n), np.zeros(n)
    cfg, st = B.CGConfig(10, 1e-6, 0, 0), B.CGStats()
    # the first two ints of SpmvAmdPrecond are kind and n (csrc/precond.hpp); kinds 2 and 3 are "chebyshev" and "multigrid"
    for kind, word in ((2, "chebyshev"), (3, "multigrid")):
        record = (C.c_int * 256)()
        record[0], record[1] = kind, n
        rc = L.spmv_amd_bicgstab_solve_device(B.Operator("stencil5-csr").op, m.ptr, C.cast(record, C.c_void_p), b.ctypes.data,
                                              x.ctypes.data, C.byref(cfg), C.byref(st))
        err = capfd.readouterr().err
        assert rc != 0 and "[BICGSTAB]" in err and word in err and "symmetric definite" in err and "refused" in err, err
    for kind in (0, 1):
        record = (C.c_int * 256)()
        record[0], record[1] = kind, n
        for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
            rc = L.spmv_amd_bicgstab_solve_device(B.Operator(mode).op, m.ptr, C.cast(record, C.c_void_p), b.ctypes.data, x.ctypes.data,
                                                  C.byref(cfg), C.byref(st))
            err = capfd.readouterr().err
            assert rc != 0 and "used before init" in err and "[BICGSTAB]" in err, (mode, err)
    # a caller's operator table (nothing to learn of its matrix): the sizes are checked between record and system
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: 1)  # never called
    record = (C.c_int * 256)()
    record[0], record[1] = 1, n - 1
    rc = L.spmv_amd_bicgstab_solve_device(C.pointer(own), m.ptr, C.cast(record, C.c_void_p), b.ctypes.data, x.ctypes.data, C.byref(cfg),
                                          C.byref(st))
    err = capfd.readouterr().err
    assert rc != 0 and "[BICGSTAB]" in err and f"the preconditioner is for {n - 1} rows" in err, err
    empty = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), 0, 0, -1)
    rc = L.spmv_amd_bicgstab_solve_device(C.pointer(own), empty.ptr, C.cast(record, C.c_void_p), b.ctypes.data, x.ctypes.data,
                                          C.byref(cfg), C.byref(st))
    err = capfd.readouterr().err
    assert rc != 0 and "[BICGSTAB]" in err and "mat->rows < 1" in err, err
    assert np.all(x == 0.0)


def test_bicgstab_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_bicgstab_stage (LAB build, include/spmv_amd/lab.h): an unknown stage or kind, null arguments, n < 1, count < 1, a
    null or misaligned pointer the stage needs -- each refused before any HIP call, non-zero, with a sentence on stderr. The
    pointers are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.BicgstabStageArgs(n=5, b=good, dinv=good, x=good, r=good, rhat=good, p=good, phat=good, shat=good, v=good, t=good,
                                   partials=good, count=3, which=4, tol=1e-6, hist=good, hist_cap=4)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(stage, kind, a, sc, word):
        rc = Blab.bicgstab_stage(stage, kind, a, sc)
        err = capfd.readouterr().err
        assert rc != 0 and "[BICGSTAB]" in err and "refused" in err and word in err, (stage, kind, word, rc, err)

    sc = Blab.BicgstabScalars()
    for stage in (None, "", "Init", "update", "step", "update_r"):
        refused(stage, "jacobi", args(), sc, "stage")
    # the vectors a stage needs under kind "jacobi"; under "none" dinv, phat and shat are not looked at (update_xr reads p instead)
    needs = {"init": ("b", "v", "dinv", "r", "rhat", "p", "phat"), "dot_rv": ("rhat", "v"), "update_s": ("v", "dinv", "r", "shat"),
             "dot_t": ("t", "r"), "update_xr": ("x", "r", "t", "rhat", "phat", "shat"), "direction": ("p", "v", "r", "dinv", "phat")}
    for stage, vectors in needs.items():
        refused(stage, "jacobi", None, sc, "null arguments")
        if stage not in ("dot_rv", "dot_t"):
            for kind in (None, "", "ilu0", "Jacobi", "chebyshev"):
                refused(stage, kind, args(), sc, "kind")
        refused(stage, "jacobi", args(n=0), sc, "n < 1")
        for name in vectors:
            for kind in ("jacobi", "none"):
                if kind == "none" and name in ("dinv", "phat", "shat"):
                    continue  # not looked at
                refused(stage, kind, args(**{name: None}), sc, name + " is null")
                refused(stage, kind, args(**{name: odd}), sc, name + " is not 16-byte aligned")
        if stage == "update_xr":
            refused(stage, "none", args(p=None), sc, "p is null")
        if stage != "direction":
            refused(stage, "none", args(partials=None), sc, "partials is null")
            refused(stage, "none", args(partials=crooked), sc, "partials is not 8-byte aligned")
        if stage not in ("init", "dot_rv"):
            refused(stage, "none", args(), None, "scalar record")
    refused("reduce", None, None, sc, "null arguments")
    refused("reduce", None, args(), None, "scalar record")
    for count in (0, -1):
        refused("reduce", None, args(count=count), sc, "count < 1")
    for which in (-1, 5):
        refused("reduce", None, args(which=which), sc, "which")
    refused("reduce", None, args(hist_cap=-1), sc, "hist_cap")
    refused("reduce", None, args(partials=None), sc, "partials is null")
    refused("reduce", None, args(partials=crooked), sc, "partials is not 8-byte aligned")
    refused("reduce", None, args(hist=None), sc, "hist is null")
    refused("reduce", None, args(hist=crooked), sc, "hist is not 8-byte aligned")
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        __import__("conftest").load_binding().bicgstab_stage("reduce", None, args(), sc)
