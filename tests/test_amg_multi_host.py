"""The AMG hierarchy with block vectors (spmv_amd_precond_create_amg_multi: csrc/amg.hip, csrc/amg_multi.hip),
CPU side: the creator is declared, exported and bound and the stage hook exists in the LAB build only; every refusal that needs no
device holds before any HIP call with its sentence and *bad_row = -1; and the one-column restatement
(tests/pcg_multi_amg_restatement.py: every level's product the sequential chain) takes the iteration counts of amg_restatement's table
in two CPU roundings, names the variant every level's single-vector product runs -- which says where single and batched bits must
coincide --, and on the 33 x 33 Poisson matrix IS amg_restatement.exact_cycle bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_restatement as AMG
import chebyshev_restatement as CH
import gcr_restatement as GR
import pcg_multi_amg_restatement as PA
from bitwise import same_bits
from conftest import ROOT

CREATOR = "spmv_amd_precond_create_amg_multi"
HOOK = "spmv_amd_amg_multi_stage"


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
    assert callable(B.Precond.amg_multi) and callable(B.amg_multi_stage)
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.amg_multi_stage("prolong_correct", 1, B.AmgStageArgs())


def test_the_creator_refuses_without_touching_the_gpu(B, capfd):
    """spmv_amd_precond_create_amg's refusals with their sentences in its order, max_rhs beside the other argument checks: behind
    theta, in front of every look at the operator. None reaches a HIP call."""
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()  # free() of an operator that was never initialised touches no device memory
    L = B._pcg_lib()
    bad = C.c_int(7)
    csr = B.Operator("cusparse-csr").op

    def refused(word, op, nu=1, max_levels=0, strength=0.08, max_rhs=4, bad_row=bad):
        bad.value = 7
        capfd.readouterr()
        got = getattr(L, CREATOR)(op, nu, max_levels, strength, max_rhs, None if bad_row is None else C.byref(bad_row))
        err = capfd.readouterr().err
        assert not got and (bad_row is None or bad.value == -1), (word, got, bad.value)
        assert "[PCG] amg:" in err or "[PCG] operator" in err, (word, err)
        assert word in err and err.count("\n") == 1, (word, err)

    refused("null operator", None)
    for nu in (-1, 9):
        refused("smoother degree", csr, nu=nu)
    for max_levels in (-1, 33):
        refused("max_levels", csr, max_levels=max_levels)
    for strength in (float("nan"), 1.0, float("inf"), -0.1):
        refused("strength", csr, strength=strength)
    for max_rhs in (0, 9, -1, -2 ** 31, 2 ** 31 - 1):
        refused("max_rhs", csr, max_rhs=max_rhs)
        refused(f"max_rhs {max_rhs} is outside 1..8", B.Operator("stencil5-csr").op, max_rhs=max_rhs)  # before the operator is looked at
    refused("smoother degree", csr, nu=9, max_levels=33, strength=1.0, max_rhs=0)  # the single creator's order: nu first,
    refused("max_levels", csr, max_levels=33, strength=1.0, max_rhs=0)             # then max_levels,
    refused("strength", csr, strength=1.0, max_rhs=0)                              # then theta, then max_rhs
    for mode in ("stencil5-csr", "stencil7-csr", "ellpack", "stencil5-ellpack"):  # not cusparse-csr: the sentence names the operator
        refused(f"operator '{mode}' is not cusparse-csr", B.Operator(mode).op)
    for nu, max_levels, strength, max_rhs in ((0, 0, 0.0, 1), (1, 1, 0.08, 3), (8, 32, 0.99, 8)):  # cusparse-csr used before init
        refused("used before init", csr, nu=nu, max_levels=max_levels, strength=strength, max_rhs=max_rhs)
    refused("used before init", csr, bad_row=None)  # bad_row may be NULL
    for max_rhs in (0, 9):
        with pytest.raises(ValueError) as info:
            B.Precond.amg_multi(B.Operator("cusparse-csr"), 1, 0, 0.08, max_rhs)
        assert info.value.bad_row == -1
    assert L.spmv_amd_precond_multigrid_max_rhs(None) == 0
    capfd.readouterr()


def test_the_stage_hook_refuses_without_touching_the_gpu(Blab, capfd):
    """k outside 1..8, then spmv_amd_amg_stage's own checks with its sentences, and a block vector that is 8 bytes off under an even
    k. The pointers are never dereferenced."""
    good, odd = 4096, 4096 + 8

    def args(**kw):
        a = Blab.AmgStageArgs(rows=4, cols=4, coarse_rows=2, row_ptr=good, col_idx=good, values=good, agg_ptr=good, members=good, agg=good,
                              z=good, r=good, coarse=good)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def refused(stage, k, a, word):
        capfd.readouterr()
        assert Blab.amg_multi_stage(stage, k, a) != 0
        err = capfd.readouterr().err
        assert "[PCG] amg: stage" in err and word in err, (stage, k, word, err)

    for k in (0, 9, -1):
        refused("residual_restrict", k, args(), "k is not 1 to 8")
    refused("smooth", 2, args(), "unknown")
    refused(None, 2, args(), "none named")
    refused("residual_restrict", 2, None, "null arguments")
    refused("prolong_correct", 2, args(rows=0), "below 1")
    refused("residual_restrict", 2, args(values=None), "CSR array")
    refused("residual_restrict", 2, args(members=None), "member list")
    refused("prolong_correct", 2, args(agg=None), "aligned")
    for stage, name in (("residual_restrict", "z"), ("residual_restrict", "r"), ("residual_restrict", "coarse"), ("prolong_correct", "z"),
                        ("prolong_correct", "coarse")):
        refused(stage, 2, args(**{name: odd}), "16-byte where k is even")
        refused(stage, 3, args(**{name: odd + 4}), "8-byte aligned")
        refused(stage, 3, args(**{name: None}), "8-byte aligned")


# ---------------------------------------------------------------- the restatement
# (system, the count of amg_restatement.TABLE at nu = 1, the variant of every level's single-vector product)
ROWS = [("poisson33", 12, ["stream", "stream", "stream"]), ("nine24", 9, ["stream", "stream"]), ("cube9", 8, ["stream", "stream", "stream"])]


@pytest.mark.parametrize("name,iterations,variants", ROWS, ids=[r[0] for r in ROWS])
def test_the_sequential_chain_cycle_takes_the_table_counts_in_two_roundings(name, iterations, variants):
    """The batched column (every level the oracle's sequential chain, every update an fma, the batched dot shape) and the same cycle
    in plain numpy (a * b + c rounded twice, dots by numpy) take the count amg_restatement.TABLE holds for the single-vector form."""
    assert {(n, nu): its for n, nu, its in AMG.TABLE}[(name, 1)] == iterations
    M, st = AMG.system(name)
    levels = AMG.hierarchy(M, 1, levels=st)
    assert PA.level_variants(levels) == variants and PA.bits_coincide(levels), name
    b, x0 = AMG.vectors(name)
    x1, h1, it1, conv1, broke1 = PA.solve_levels(levels, b, x0)
    products = PA.chains(levels)
    x2, h2, it2, conv2 = CH._loop(products[0], lambda u, v: float(u @ v), b, x0, AMG.make_cycle(levels, products, products), 1e-6, 1000)
    print(f"{name}: {it1} / {it2} iterations, last {h1[-1] / h1[0]:.3e} / {h2[-1] / h2[0]:.3e}")
    assert conv1 and conv2 and not broke1 and it1 == it2 == iterations, (name, it1, it2)
    assert np.linalg.norm(b - AMG.scipy_of(M) @ x1) < 1e-6 * h1[0] * (1.0 + 1e-6)


def test_gcr_on_the_upwind_stencil_in_two_roundings():
    name, nu, restart, iterations = AMG.GCR_ROW
    M, b, x0 = AMG.upwind33()
    levels = AMG.hierarchy(M, nu)
    assert PA.level_variants(levels) == ["stream", "stream", "stream"]
    products = PA.chains(levels)
    r1 = PA.gcr_levels(levels, b, x0, restart)
    r2 = GR.gcr(AMG.scipy_of(M), b, x0, AMG.make_cycle(levels, products, products), restart)
    assert r1[2] == r2[2] == iterations == 10 and r1[3] and r2[3], (r1[2:4], r2[2:4])
    assert GR.hist_err(r1[1], r2[1]) < 1e-10


def test_where_single_and_batched_bits_coincide(O):
    """Poisson 33 x 33: every level's single-vector product is csr/stream, whose row sum IS the sequential chain, so the batched cycle
    equals amg_restatement.exact_cycle bit for bit (nu = 0, 1, 2). The arrow at theta = 0: level 0 runs csr/adaptive (hub rows of 2 501
    entries summed as a tree), so there the two cycles are two roundings of one cycle: equal to 1e-12 of |z|, and not bit for bit."""
    M, st = AMG.system("poisson33")
    r = np.random.default_rng(26).standard_normal(AMG.rows_of(M))
    for nu in (0, 1, 2):
        levels = AMG.hierarchy(M, nu, levels=st)
        assert PA.bits_coincide(levels)
        assert same_bits(PA.make_cycle(levels)(r), AMG.exact_cycle(O, levels)(r)), nu
    levels = AMG.hierarchy(AMG.arrow(), 1, 0, 0.0)
    assert PA.level_variants(levels) == ["adaptive", "stream"] and not PA.bits_coincide(levels)
    r = np.random.default_rng(27).standard_normal(levels[0].rows)
    chain, tree = PA.make_cycle(levels)(r), AMG.exact_cycle(O, levels)(r)
    assert np.linalg.norm(chain - tree) <= 1e-12 * np.linalg.norm(tree) and not same_bits(chain, tree)
