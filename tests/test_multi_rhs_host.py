"""Several right-hand sides per matrix pass, CPU side: the new entry points are exported by the product library and declared in
api.h, and their argument checks refuse bad calls before any HIP call -- so they hold on a machine without a GPU. So do the
refusals of the LAB build's stage hook (spmv_amd_cg_multi_stage), and the numpy restatement of the dot partials that
tests/test_multi_rhs_stages_gpu.py compares the kernels with is held against math.fsum here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import multi_rhs_restatement as R
from conftest import ROOT

SUM_TOL = 1e-13  # a re-ordered fp64 sum against math.fsum, of sum|terms| (tests/test_blas1_gpu.py, test_pcg_stages_gpu.py)

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


def test_the_stage_hook_is_a_lab_symbol_only(B, Blab):
    name = "spmv_amd_cg_multi_stage"
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    assert name in B.LAB_ONLY_SYMBOLS and name not in B.DECLARED_SYMBOLS and name not in NEW
    assert not hasattr(B.lib(), name) and hasattr(Blab.lib(), name)
    assert name not in open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    assert re.search(r"\b" + name + r"\s*\(", open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read())
    assert name not in open(os.path.join(csrc, "exports.map")).read()
    assert re.search(r"^\s+" + name + r";", open(os.path.join(csrc, "exports_lab.txt")).read(), flags=re.M)
    assert C.sizeof(B.MultiColumn) == 64 and B.MultiColumn.active.offset == 48 and B.MultiColumn.iterations.offset == 56
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.cg_multi_stage("reduce", 1, B.CgMultiStageArgs())


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory (nothing to release): safe without a GPU, and
    # it makes "used before init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack"):
        B.Operator(mode).free()


def test_spmm_argument_checks_refuse_without_touching_the_gpu(B, capfd):
    """Each refusal of the operand entry points is non-zero and says why on stderr, under the tag it has always had: the number of
    right-hand sides and the operator under [multi-rhs], the block vectors under [CG-MULTI]."""
    _free_all(B)
    L = B._multi_lib()
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)

    def refused(rc, tag, word):
        err = capfd.readouterr().err
        assert rc != 0 and tag in err and word in err, (tag, word, rc, err)

    for k in (0, -1, 9, 100):
        refused(L.spmv_amd_spmm_device(b"stencil5-csr", k, p, p), "[multi-rhs]", "right-hand sides")
    refused(L.spmv_amd_spmm_device(b"stencil5-csr", 2, None, p), "[CG-MULTI]", "null block vector")
    refused(L.spmv_amd_spmm_device(b"stencil5-csr", 2, p, None), "[CG-MULTI]", "null block vector")
    assert L.spmv_amd_spmm_device(None, 2, p, p) != 0
    refused(L.spmv_amd_spmm_device(b"no-such-operator", 2, p, p), "[multi-rhs]", "unknown operator 'no-such-operator'")
    refused(L.spmv_amd_spmm_device(b"ellpack", 2, p, p), "[multi-rhs]", "no multi-RHS path")
    refused(L.spmv_amd_spmm_device(b"stencil5-ellpack", 2, p, p), "[multi-rhs]", "stencil5-csr, stencil7-csr and cusparse-csr have one")
    refused(L.spmv_amd_spmm_device(b"stencil5-csr", 2, p, p), "[multi-rhs]", "used before init")
    refused(L.spmv_amd_spmm_device(b"cusparse-csr", 1, p, p), "[multi-rhs]", "used before init")
    refused(L.spmv_amd_spmm_device(b"stencil5-csr", 2, C.c_void_p(p.value + 4), p), "[CG-MULTI]", "8-byte aligned")
    refused(L.spmv_amd_spmm_device(b"stencil5-csr", 2, p, C.c_void_p(p.value + 4)), "[CG-MULTI]", "8-byte aligned")
    assert L.spmv_amd_spmm_variant(b"ellpack") == b"none"
    assert L.spmv_amd_spmm_variant(b"stencil5-csr") == b"uninitialised"
    assert L.spmv_amd_spmm_variant(b"nope") == b"unknown-operator"
    assert L.spmv_amd_block_to_device(0, 4, p, p) != 0 and L.spmv_amd_block_to_device(9, 4, p, p) != 0
    refused(1, "[multi-rhs]", "right-hand sides")
    assert L.spmv_amd_block_to_host(2, 4, None, p) != 0 and L.spmv_amd_block_to_host(2, 4, p, None) != 0
    refused(1, "[CG-MULTI]", "null block vector")


def test_cg_multi_argument_checks_refuse_without_touching_the_gpu(B, capfd):
    """Each refusal is non-zero and says why on stderr: the number of right-hand sides and the operator under [multi-rhs], the rest
    under [CG-MULTI]. max_iters < 0 is refused before the operator is looked at (the order of the batched solvers' shared checks,
    csrc/multi_solve.hpp); tests/test_multi_rhs_gpu.py holds the same sentence on an initialised operator."""
    _free_all(B)
    L = B._multi_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    Bk = np.ones((9, n))
    X = np.zeros((9, n))
    cfg = B.CGConfig(10, 1e-6, 0, 0)
    stats = (B.CGStats * 9)()

    def refused(op, k, tag, word, mat=m.ptr, b=Bk.ctypes.data, x=X.ctypes.data, c=C.byref(cfg), s=stats):
        rc = L.spmv_amd_cg_solve_device_multi(op, mat, k, b, x, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and tag in err and word in err, (k, tag, word, rc, err)

    stencil = B.Operator("stencil5-csr").op
    for k in (0, 9, -3):
        refused(stencil, k, "[multi-rhs]", "right-hand sides")
    refused(stencil, 2, "[CG-MULTI]", "null argument", mat=None)
    refused(stencil, 2, "[CG-MULTI]", "null argument", b=None)
    refused(stencil, 2, "[CG-MULTI]", "null argument", x=None)
    refused(stencil, 2, "[CG-MULTI]", "null argument", c=None)
    refused(stencil, 2, "[CG-MULTI]", "null argument", s=None)
    refused(None, 2, "[CG-MULTI]", "null operator")
    refused(stencil, 2, "[CG-MULTI]", "max_iters < 0", c=C.byref(B.CGConfig(-1, 1e-6, 0, 0)))
    for mode in ("ellpack", "stencil5-ellpack"):
        refused(B.Operator(mode).op, 2, "[multi-rhs]", "no multi-RHS path")
        refused(B.Operator(mode).op, 2, "[multi-rhs]", "'" + mode + "' has no multi-RHS path (stencil5-csr, stencil7-csr and cusparse-csr have one)")
    refused(stencil, 2, "[multi-rhs]", "'stencil5-csr' used before init")
    refused(B.Operator("stencil7-csr").op, 2, "[multi-rhs]", "'stencil7-csr' used before init")
    refused(B.Operator("cusparse-csr").op, 1, "[multi-rhs]", "used before init")
    own = B.SpmvOperator()                                               # a caller's own vtable
    own.name = b"mine"
    refused(C.pointer(own), 2, "[multi-rhs]", "no multi-RHS path")
    with pytest.raises(RuntimeError):
        B.cg_solve_multi(B.Operator("stencil5-csr"), m, np.ones((2, n)), np.zeros((2, n)))
    # columns that no batched solve can have had; no workspace once the operators are freed
    assert L.spmv_amd_cg_last_history_multi(-1, None, 0) == -1
    assert L.spmv_amd_cg_last_history_multi(8, None, 0) == -1
    assert L.spmv_amd_cg_multi_workspace_bytes() == 0


# ---------------------------------------------------------------- the restatement of the dot partials
def _fsum_blocks(p, layout):
    """math.fsum of each workgroup's products and of their absolute values, by plain indexing (no reshaping tricks)."""
    sums, mags = [], []
    if layout[0] == "flat":
        for lo in range(0, len(p), 256):
            sums.append(math.fsum(p[lo:lo + 256])), mags.append(math.fsum(np.abs(p[lo:lo + 256])))
    else:
        n = layout[1]
        for gi in range(n):
            for lo in range(0, n, 256):
                part = p[gi * n + lo:gi * n + min(lo + 256, n)]
                sums.append(math.fsum(part)), mags.append(math.fsum(np.abs(part)))
    return np.array(sums), np.array(mags)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_restatement_flat_against_fsum(rows):
    p = np.random.default_rng(rows).standard_normal(rows) * np.random.default_rng(rows + 1).standard_normal(rows)
    got = R.block_partials_of(p, R.flat())
    want, mag = _fsum_blocks(p, R.flat())
    assert len(got) == R.block_count(rows, R.flat()) == (rows + 255) // 256 == len(want)
    assert np.all(np.abs(got - want) <= SUM_TOL * mag)


@pytest.mark.parametrize("n", [1, 3, 65, 256, 257, 513, 576])
def test_restatement_grid_against_fsum(n):
    p = np.random.default_rng(n).standard_normal(n * n)
    got = R.block_partials_of(p, R.grid(n))
    want, mag = _fsum_blocks(p, R.grid(n))
    assert len(got) == R.block_count(n * n, R.grid(n)) == n * ((n + 255) // 256) == len(want)
    assert np.all(np.abs(got - want) <= SUM_TOL * mag)


def test_restatement_shape_is_the_kernels():
    """Powers of two far apart make the order of the additions visible: lane 0 of a wave is ((v0 + v32) + (v16 + v48)) + ..., and
    the four waves are summed ((w0 + w1) + w2) + w3, not pairwise."""
    v = np.zeros(256)
    v[0], v[64], v[128], v[192] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53   # (1 + e) + e + e = 1; 1 + (e + e) would be 1 + 2e
    assert R.block_partials_of(v, R.flat())[0] == 1.0
    v[0], v[64], v[128], v[192] = 2.0 ** -53, 2.0 ** -53, 1.0, 0.0           # (e + e) + 1 = 1 + 2e
    assert R.block_partials_of(v, R.flat())[0] == 1.0 + 2.0 ** -52
    w = np.zeros(256)
    w[0], w[1], w[2] = 1.0, 2.0 ** -53, 2.0 ** -53  # lanes 1 and 2 meet lane 0 separately: (1 + e) ... + e = 1
    assert R.block_partials_of(w, R.flat())[0] == 1.0
    w[0], w[32], w[1], w[33] = 0.0, 1.0, 2.0 ** -53, 2.0 ** -53  # lanes 1 and 33 meet first: (0 + 1) + (e + e)
    w[2] = 0.0
    assert R.block_partials_of(w, R.flat())[0] == 1.0 + 2.0 ** -52


def test_restatement_dead_positions_contribute_nothing():
    rng = np.random.default_rng(3)
    for rows in (1, 65, 257, 1000):
        p = rng.standard_normal(rows)
        padded = np.concatenate([p, np.zeros(-rows % 256)])
        assert np.array_equal(R.block_partials_of(p, R.flat()), R.block_partials_of(padded, R.flat()))
    for n in (3, 65, 257):  # a grid row's dead columns: the same partials as the rows laid out with explicit zeros
        p = rng.standard_normal(n * n)
        cb = (n + 255) // 256
        padded = np.zeros((n, cb * 256))
        padded[:, :n] = p.reshape(n, n)
        assert np.array_equal(R.block_partials_of(p, R.grid(n)), R.block_partials_of(padded.ravel(), R.flat()))
        assert np.all(R.positions(p, R.grid(n)).reshape(n, -1)[:, n:] == 0.0)


def test_restatement_layouts_agree_on_multiples_of_256():
    for n in (256, 512):
        p = np.random.default_rng(n).standard_normal(n * n)
        assert np.array_equal(R.block_partials_of(p, R.grid(n)), R.block_partials_of(p, R.flat()))


# ---------------------------------------------------------------- the LAB build's stage hook
def test_cg_multi_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_cg_multi_stage (LAB build, include/spmv_amd/lab.h): an unknown stage, k outside 1..8, null arguments, a null or
    misaligned pointer the stage needs, n < 1, count < 1, which outside 0..2, hist_cap < 0, an operator that is unknown,
    uninitialised or without a multi-RHS path -- each refused before any HIP call, non-zero, with a sentence on stderr. The
    pointers are never dereferenced."""
    _free_all(Blab)
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def args(**kw):
        a = Blab.CgMultiStageArgs(mode=b"stencil5-csr", n=5, X=good, R=good, P=good, AP=good, cols=good, partials=good, count=3, which=2,
                                  tol=1e-6, hist=good, hist_cap=4, xcd_run=0)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, k, a, word):
        rc = Blab.cg_multi_stage(stage, k, a)
        err = capfd.readouterr().err
        assert rc != 0 and "[CG-MULTI]" in err and "refused" in err and word in err, (stage, k, word, rc, err)

    for stage in (None, "", "Init", "update", "step", "spmv"):
        refused(stage, 2, args(), "stage")
    needs = {"init": ("AP", "R", "P"), "update_r": ("AP", "R"), "update_xp": ("R", "P", "X")}
    for stage in ("spmm", "init", "update_r", "update_xp", "reduce"):
        for k in (0, -1, 9, 100):
            refused(stage, k, args(), "k is not 1 to 8")
        refused(stage, 2, None, "null arguments")
    for stage, vectors in needs.items():
        for k in (1, 2, 5, 8):
            refused(stage, k, args(n=0), "n < 1")
            for name in vectors:
                refused(stage, k, args(**{name: None}), name + " is null")
                refused(stage, k, args(**{name: odd}), name + " is not 16-byte aligned")
        if stage != "update_xp":
            refused(stage, 2, args(partials=None), "partials is null")
            refused(stage, 2, args(partials=crooked), "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, 2, args(cols=None), "cols is null")
            refused(stage, 2, args(cols=crooked), "cols is not 8-byte aligned")
    for count in (0, -1):
        refused("reduce", 2, args(count=count), "count < 1")
    for which in (-1, 3):
        refused("reduce", 2, args(which=which), "which")
    refused("reduce", 2, args(hist_cap=-1), "hist_cap < 0")
    refused("reduce", 2, args(which=0, hist_cap=0), "hist_cap < 1")
    refused("reduce", 2, args(partials=None), "partials is null")
    refused("reduce", 2, args(partials=crooked), "partials is not 8-byte aligned")
    refused("reduce", 2, args(cols=None), "cols is null")
    refused("reduce", 2, args(hist=None), "hist is null")
    refused("reduce", 2, args(hist=crooked), "hist is not 8-byte aligned")
    for name in ("X", "AP"):
        refused("spmm", 2, args(**{name: None}), name + " is null")
        refused("spmm", 2, args(**{name: crooked}), name + " is not 8-byte aligned")
    refused("spmm", 2, args(partials=crooked), "partials is not 8-byte aligned")
    refused("spmm", 2, args(xcd_run=-1), "xcd_run < 0")
    refused("spmm", 2, args(mode=None), "no operator named")
    refused("spmm", 2, args(mode=b"no-such-operator"), "unknown operator")
    for mode in (b"ellpack", b"stencil5-ellpack"):
        refused("spmm", 2, args(mode=mode), "no multi-RHS path")
    for mode in (b"stencil5-csr", b"cusparse-csr"):
        refused("spmm", 2, args(mode=mode, X=odd, AP=odd), "used before init")  # 8-byte alignment is enough for the SpMM
