"""The LAB build's spmv_amd_operator_fused_spmv on the CPU: it is a symbol of the LAB library only, declared in lab.h and listed, and
its argument checks refuse bad calls before any HIP call (so they hold on a machine without a GPU), each with a sentence on stderr.
The refusals that need an initialised operator (no fused form, cap below the partial count) are in tests/test_csr_gpu.py."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HOOK = "spmv_amd_operator_fused_spmv"
OPERATORS = ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack")


def test_the_hook_is_a_symbol_of_the_lab_library_only(B, Blab):
    csrc = os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc")
    exports, exports_lab = open(os.path.join(csrc, "exports.map")).read(), open(os.path.join(csrc, "exports_lab.txt")).read()
    lab_h = open(os.path.join(ROOT, "include", "spmv_amd", "lab.h")).read()
    api_h = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    assert HOOK in B.LAB_ONLY_SYMBOLS and HOOK not in B.DECLARED_SYMBOLS
    assert hasattr(Blab.lib(), HOOK) and not hasattr(B.lib(), HOOK)
    assert re.search(r"\b" + HOOK + r"\s*\(", lab_h) and HOOK not in api_h
    assert re.search(r"^\s+" + HOOK + r";", exports_lab, flags=re.M) and HOOK not in exports
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        B.fused_spmv(B.Operator("cusparse-csr"), 4096, 4096, 4096, 1)


def test_fused_spmv_refuses_without_touching_the_gpu(Blab, capfd):
    """Null arguments, a table this library does not own and every operator before its init. The pointers are never dereferenced."""
    for mode in OPERATORS:  # free() of an operator that was never initialised touches no device memory
        Blab.Operator(mode).free()
    good = 4096
    csr = Blab.Operator("cusparse-csr")

    def refused(word, op, x=good, y=good, partials=good, cap=1 << 20, count=True):
        capfd.readouterr()
        rc, used = Blab.fused_spmv(op, x, y, partials, cap, count)
        err = capfd.readouterr().err
        assert rc != 0 and used == -1 and "[fused-spmv]" in err and "refused" in err and word in err, (word, rc, used, err)
        assert err.count("\n") == 1  # one sentence

    refused("null arguments", None)
    refused("null arguments", csr, x=None)
    refused("null arguments", csr, y=None)
    refused("null arguments", csr, partials=None)
    refused("null arguments", csr, count=False)
    own = Blab.SpmvOperator()  # a caller's own vtable
    own.name = b"mine"
    refused("not one of this library's tables", C.pointer(own))
    for mode in OPERATORS:
        refused("before init", Blab.Operator(mode))
        refused("before init", Blab.Operator(mode), cap=0)  # asked before the partial count is known
