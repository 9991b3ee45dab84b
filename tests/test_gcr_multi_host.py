"""Batched GCR(m), CPU side: the entry points are exported, declared and listed, the LAB build's stage hook is in the LAB build only,
every refusal that needs no device holds before any HIP call, spmv_amd_gcr_multi_workspace_bytes is the stated arithmetic, and the
INPUTS of the GPU tests are sound: on every row of gcr_multi_restatement.TABLE the two CPU roundings of gcr_restatement agree on the
iteration count and the ending, the stored figure is what they disagree by (computed here), and the restatement of one column
(tests/gcr_multi_restatement.py: the batched dot shape, the oracle's fma, the operator's own product, the application in the library's
bits) takes that count and ending and agrees with plain numpy within the row's third-rounding bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gcr_multi_restatement as GM
import gcr_restatement as GR
from conftest import ROOT
from gcr_restatement import entries_of, hist_err, table_system, third_rounding_bound, true_residual_norm

NEW = ["spmv_amd_gcr_solve_device_multi", "spmv_amd_gcr_last_history_multi", "spmv_amd_gcr_multi_workspace_bytes"]
HOOK = "spmv_amd_gcr_multi_stage"
STAGES = ("init", "multidot", "orthogonalise", "update_xr")


def test_gcr_multi_symbols_exported_declared_and_listed(B, Blab):
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
    for word in ("SpmvAmdGcrMultiColumn", "SpmvAmdGcrMultiStageArgs"):
        assert word in lab and word not in api
    col = B.GcrMultiColumn
    assert C.sizeof(col) == 560 and col.beta.offset == 256 and col.alpha.offset == 512 and col.done.offset == 544 and col.breakdown.offset == 556
    assert f"#define SPMV_AMD_GCR_MULTI_DOT_CHUNK {B.GCR_MULTI_DOT_CHUNK} " in lab and f"#define SPMV_AMD_GCR_MULTI_ORTH_CHUNK {B.GCR_MULTI_ORTH_CHUNK} " in lab
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.gcr_multi_stage("reduce", "none", 1, B.GcrMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_gcr_multi_argument_checks_refuse_without_touching_the_gpu(B, capfd):
    """nrhs outside 1..8, restart outside 0..32, a null argument, max_iters < 0, an operator without a multi-RHS path, a caller's own
    table, an operator used before init: each refused before any HIP call, non-zero, with a [GCR-MULTI] sentence in the words of the
    other batched entry points. The handle is a record of zeros (kind "none") that no later check reaches; a real one needs a device
    (its refusals: tests/test_gcr_multi_gpu.py)."""
    _free_all(B)
    L = B._gcr_multi_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    Bk, X = np.ones((9, n)), np.zeros((9, n))
    cfg = B.CGConfig(10, 1e-6, 0, 0)
    stats = (B.CGStats * 9)()
    record = (C.c_int * 1024)()
    handle = C.cast(record, C.c_void_p)

    def refused(op, k, restart=4, mat=m.ptr, pc=handle, b=Bk.ctypes.data, x=X.ctypes.data, c=C.byref(cfg), s=stats, word=""):
        rc = L.spmv_amd_gcr_solve_device_multi(op, mat, pc, restart, k, b, x, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and "[GCR-MULTI]" in err and word in err, (k, restart, word, rc, err)

    stencil = B.Operator("stencil5-csr").op
    for k in (0, 9, -3, 100):
        refused(stencil, k, word=f"nrhs = {k}: 1 to 8 right-hand sides are supported")
    for restart in (-1, 33, 1000):
        refused(stencil, 2, restart=restart, word=f"restart = {restart}: 1 .. 32, or 0 for the default 16: refused")
    refused(stencil, 2, mat=None, word="null argument")
    refused(stencil, 2, pc=None, word="null argument")
    refused(stencil, 2, b=None, word="null argument")
    refused(stencil, 2, x=None, word="null argument")
    refused(stencil, 2, c=None, word="null argument")
    refused(stencil, 2, s=None, word="null argument")
    refused(None, 2, word="null argument")
    refused(stencil, 2, c=C.byref(B.CGConfig(-1, 1e-6, 0, 0)), word="max_iters < 0")
    for mode in ("ellpack", "stencil5-ellpack"):
        refused(B.Operator(mode).op, 2, word="has no multi-RHS path (stencil5-csr, stencil7-csr and cusparse-csr have one)")
    own = B.SpmvOperator()  # a caller's own vtable
    own.name = b"mine"
    refused(C.pointer(own), 2, word="no multi-RHS path")
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr"):
        for restart in (0, 1, 32):
            refused(B.Operator(mode).op, 1, restart=restart, word="used before init")
    assert np.all(X == 0.0)
    assert L.spmv_amd_gcr_last_history_multi(-1, None, 0) == -1
    assert L.spmv_amd_gcr_last_history_multi(8, None, 0) == -1


def test_gcr_multi_workspace_bytes_is_the_stated_arithmetic(B):
    """(4 + 2 m) block vectors, two more for "chebyshev" and "multigrid", 32 k partial rows of (rows + 255) / 256 doubles; one unit of
    restart costs 16 rows k bytes; restart 0 is 16; refused arguments give 0. The issue's example: 20 000^2 rows at k = 4 and m = 16
    is about 410 GB of basis -- more than any device holds, so the solve refuses it and names a smaller restart."""
    W = B.gcr_multi_workspace_bytes
    for rows in (1, 255, 1089, 4225, 400_000_000):
        groups = (rows + 255) // 256
        for k in (1, 3, 8):
            for kind, extra in (("none", 0), ("jacobi", 0), ("chebyshev", 2), ("multigrid", 2)):
                for m in (1, 4, 16, 32):
                    assert W(rows, k, m, kind) == ((4 + extra + 2 * m) * rows * k + 32 * k * groups) * 8, (rows, k, kind, m)
                assert W(rows, k, 0, kind) == W(rows, k, 16, kind)
                assert W(rows, k, 17, kind) - W(rows, k, 16, kind) == 16 * rows * k
    rows = 20_000 * 20_000
    basis = W(rows, 4, 16, "none") - W(rows, 4, 1, "none") + 16 * rows * 4
    assert 405e9 < basis < 415e9 and W(rows, 4, 16, "none") > 288e9  # beyond an MI355X's 288 GB
    for bad in ((0, 2, 4, "none"), (-5, 2, 4, "none"), (9, 0, 4, "none"), (9, 9, 4, "none"), (9, 2, -1, "none"), (9, 2, 33, "none"),
                (9, 2, 4, "ilu"), (9, 2, 4, None), (9, 2, 4, "")):
        assert W(*bad) == 0, bad


def test_gcr_multi_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_gcr_multi_stage (LAB build): an unknown stage or kind, k outside 1..8, null arguments, a null or misaligned pointer the
    stage needs, n < 1, a slot outside the stage's range, count < 1, which outside 0..3, hist_cap < 0 -- each refused before any HIP
    call. The pointers are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that
    keep = []

    def slots(value=good, **kw):
        arr = (C.c_void_p * 32)(*([value] * 32))
        for i, v in kw.items():
            arr[int(i[1:])] = v
        keep.append(arr)
        return arr

    def args(**kw):
        a = Blab.GcrMultiStageArgs(n=5, X=good, R=good, AX=good, z_in=good, ZS=good, Q=slots(), Z=slots(), slot=3, dinv=good, cols=good,
                                   shadow=good, partials=good, count=3, which=3, tol=1e-6, hist=good, hist_cap=4)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, kind, k, a, word):
        rc = Blab.gcr_multi_stage(stage, kind, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[GCR-MULTI]" in err and "refused" in err and word in err, (stage, kind, k, word, rc, err)

    for stage in (None, "", "Init", "update", "update_r", "dot", "spmm"):
        refused(stage, "jacobi", 2, args(), "stage")
    for stage in STAGES + ("reduce",):
        for k in (0, -1, 9, 100):
            refused(stage, "jacobi", k, args(), "k is not 1 to 8")
        refused(stage, "jacobi", 2, None, "null arguments")
    needs = {"init": ("R", "AX"), "multidot": (), "orthogonalise": ("R", "z_in"), "update_xr": ("X", "R")}
    for stage, vectors in needs.items():
        if stage in ("init", "update_xr"):
            for kind in (None, "", "ilu0", "Jacobi", "chebyshev", "multigrid"):
                refused(stage, kind, 2, args(), "kind")
            refused(stage, "jacobi", 2, args(dinv=None), "dinv is null")
            refused(stage, "jacobi", 2, args(dinv=crooked), "dinv is not 8-byte aligned")
            refused(stage, "jacobi", 2, args(ZS=None), "ZS is null")
            refused(stage, "jacobi", 2, args(ZS=odd), "ZS is not 16-byte aligned")
        refused(stage, "none", 2, args(n=0), "n < 1")
        for k in (1, 2, 5, 8):
            for name in vectors:
                refused(stage, "none", k, args(**{name: None}), name + " is null")
                refused(stage, "none", k, args(**{name: odd}), name + " is not 16-byte aligned")
        refused(stage, "none", 2, args(partials=None), "partials is null")
        refused(stage, "none", 2, args(partials=crooked), "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, "none", 2, args(cols=None), "cols is null")
            refused(stage, "none", 2, args(cols=crooked), "cols is not 8-byte aligned")
            refused(stage, "none", 2, args(slot=32), "slot outside")
            refused(stage, "none", 2, args(slot=-1), "slot outside")
            refused(stage, "none", 2, args(Q=None), "Q is null")
            refused(stage, "none", 2, args(Q=slots(s3=None)), "Q[3] is null")
            refused(stage, "none", 2, args(Q=slots(s3=odd)), "Q[3] is not 16-byte aligned")
        if stage == "multidot":
            refused(stage, "none", 2, args(slot=0), "slot outside 1 .. 31")
            refused(stage, "none", 2, args(Q=slots(s0=None)), "Q[0] is null")
        if stage in ("orthogonalise", "update_xr"):
            refused(stage, "none", 2, args(Z=None), "Z is null")
            refused(stage, "none", 2, args(Z=slots(s3=odd)), "Z[3] is not 16-byte aligned")
        if stage == "orthogonalise":
            refused(stage, "none", 2, args(Z=slots(s1=None)), "Z[1] is null")
    for count in (0, -1):
        refused("reduce", None, 2, args(count=count), "count < 1")
    for which in (-1, 4):
        refused("reduce", None, 2, args(which=which), "which")
    refused("reduce", None, 2, args(which=1, slot=0), "slot outside 1 .. 31")
    refused("reduce", None, 2, args(which=2, slot=32), "slot outside 0 .. 31")
    refused("reduce", None, 2, args(hist_cap=-1), "hist_cap < 0")
    refused("reduce", None, 2, args(partials=None), "partials is null")
    refused("reduce", None, 2, args(partials=crooked), "partials is not 8-byte aligned")
    refused("reduce", None, 2, args(cols=None), "cols is null")
    refused("reduce", None, 2, args(shadow=None), "shadow is null")
    refused("reduce", None, 2, args(hist=None), "hist is null")
    refused("reduce", None, 2, args(hist=crooked), "hist is not 8-byte aligned")


# ---------------------------------------------------------------- the table
def product_of(O, name):
    """The product the GPU tests' stencil operator makes of a table system (stencil5-csr in 2-D, stencil7-csr in 3-D)."""
    A, _, _ = table_system(name)
    rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
    if GR.dimension_of(name) == 3:
        return lambda u: O.spmv_csr(rp, ci, va, u)
    grid = GR.grid_of(A, 2)
    return lambda u: O.spmv_stencil5(rp, ci, va, u, grid)


@pytest.mark.parametrize("name, kind, restart", GM.CASES, ids=[f"{c[0]}-{c[1]}-m{c[2]}" for c in GM.CASES])
def test_the_table_holds_in_every_rounding(O, name, kind, restart):
    """Seeds 0..7 of one (system, kind, restart): gcr() and gcr_other_rounding() agree on the count and the ending the table stores;
    the stored figure is twice their history disagreement (one digit, rounded up, never below 1e-14); the restatement of the column --
    in the exact form on the operator's product and with the dot shape alone in plain numpy -- takes the same count and ending, and
    its history and x lie within third_rounding_bound(stored) of gcr(); the true residual is below 1.01 tol ||r0||."""
    A, _, _ = table_system(name)
    dim = GR.dimension_of(name)
    matvec = product_of(O, name)
    exact = GR.exact_apply(O, A, dim, kind)
    plain = GR.make_apply(A, dim, kind)
    counts = set()
    for seed, (iterations, end, stored) in GM.rows_of(name, kind, restart):
        b, x0 = GM.column(name, seed)
        (x1, h1, i1, c1, e1), (_, h2, i2, c2, e2) = GM.two_roundings(name, kind, restart, seed)
        assert (i1, e1) == (i2, e2) == (iterations, end) and c1 and c2, (seed, i1, e1, i2, e2)
        err = hist_err(h1, h2)
        assert max(1e-14, 2.0 * err) <= stored <= max(1e-14, 4.0 * err), (seed, err, stored)
        bound = third_rounding_bound(stored)
        runs = {"numpy": GM.solve_numpy(A, b, x0, plain, restart), "exact": GM.solve(matvec, b, x0, exact, restart)}
        for what, (x, h, it, conv, how) in runs.items():
            e = hist_err(h, h1)
            print(f"{(name, kind, restart, seed)} {what}: {it} iterations, {how}, CPU roundings {err:.2e} (stored {stored:g}), against gcr() {e:.2e}")
            assert (it, how, conv) == (iterations, end, True) and len(h) == iterations + 1, (seed, what, it, how)
            assert e <= bound and np.max(np.abs(x - x1)) <= bound * np.max(np.abs(x1)), (seed, what, e)
            assert true_residual_norm(entries_of(A), b, x) <= 1.01 * GM.TOL * h[0], (seed, what)
        counts.add(iterations)
    assert len(counts) >= 2  # the columns of a batch stop in different iterations: the whole-solve tests exercise freezing


def test_columns_are_the_table_system_and_the_seeded_columns():
    _, b, x0 = table_system("grid33")
    assert all(np.array_equal(u, v) for u, v in zip(GM.column("grid33", 0), (b, x0)))
    rng = np.random.default_rng(1002)
    b2, x2 = GM.column("grid33", 2)
    assert np.array_equal(b2, rng.standard_normal(33 * 33)) and np.array_equal(x2, rng.standard_normal(33 * 33))
    assert len(GM.TABLE) == 8 * len(GM.CASES) and all(v[1] == "converged" for v in GM.TABLE.values())


# ---------------------------------------------------------------- every end in one batch
# A 10 x 10 block-diagonal matrix, one column supported on each block (tests/test_gcr_multi_gpu.py solves the batch on the device):
# 0 I (stored zeros): q = 0, gamma = 0. A quarter turn with b = (1, 0): q = (0, -1) is orthogonal to r, rho = 0 with gamma = 1. 2 I with
# b = (1.5, -0.75): alpha = 0.5 exactly, r = 0 -- converged in iteration 1. diag(1, 2) with b = (1, 1) at tol
# 1e-6 under restart 1 loses a factor of about sqrt(10) per iteration: converged late. diag(1, 10) with b = (1, 1) loses 9 / 11 per
# iteration: the cap ends it.
ENDS_BLOCKS = [np.zeros((2, 2)), np.array([[0.0, 1.0], [-1.0, 0.0]]), 2.0 * np.eye(2), np.diag([1.0, 2.0]), np.diag([1.0, 10.0])]
ENDS_B = np.zeros((5, 10))
for _j, _v in enumerate(([1.5, -0.75], [1.0, 0.0], [1.5, -0.75], [1.0, 1.0], [1.0, 1.0])):
    ENDS_B[_j, 2 * _j:2 * _j + 2] = _v
ENDS = ["gamma", "rho", "converged", "converged", "max_iters"]
ENDS_ITERATIONS = [1, 1, 1, 12, 16]
ENDS_CAP, ENDS_TOL, ENDS_RESTART = 16, 1e-6, 1


def ends_entries():
    """(row, col, value) of the block matrix, zeros of the first block stored, sorted by row and column."""
    out = []
    for j, blk in enumerate(ENDS_BLOCKS):
        for r in range(2):
            for c in range(2):
                if blk[r, c] != 0.0 or (j == 0 and r == c):
                    out.append((2 * j + r, 2 * j + c, float(blk[r, c])))
    return out


def test_every_end_in_one_batch_on_the_cpu(O, B):
    e = np.zeros(len(ends_entries()), dtype=B.ENTRY_DTYPE)
    for i, v in enumerate(ends_entries()):
        e[i] = v
    rp, ci, va = O.build_csr(e, 10)
    for j, (end, its) in enumerate(zip(ENDS, ENDS_ITERATIONS)):
        x, h, it, conv, how = GM.solve(lambda u: O.spmv_csr(rp, ci, va, u), ENDS_B[j], np.zeros(10), lambda r: r, ENDS_RESTART, ENDS_TOL, ENDS_CAP)
        assert (how, it, conv) == (end, its, end == "converged"), (j, how, it)
        assert len(h) == it + 1 and np.all(np.isfinite(x))
        if end in ("gamma", "rho"):
            assert np.array_equal(x, np.zeros(10)) and h[1] == h[0] > 0.0
