"""What the three single-vector preconditioned solves print on stdout, line by line: a verbose = 2 solve of each on stencil5-csr
(init_synthetic(8): 64 rows, b = 1, x0 = 0) and one breakdown system each, taken from the suite (tests/test_pcg_gpu.py,
test_bicgstab_gpu.py, test_gcr_gpu.py). The verdict and the time breakdown come from one shared function (csrc/single_solve.hpp)
that takes the solver's tag and the name of its breakdown scalar; the expected text below is what the solvers printed while each
still had its own copy of those lines, checked against their printf calls. The four time values are masked."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIMES = re.compile(r"^(     (?:Total|SpMV|BLAS1|Reductions): +)[0-9.]+ ms$", flags=re.M)


def stdout_of(call):
    """What `call` writes to file descriptor 1, the library's buffered printf included."""
    libc = C.CDLL(None)
    libc.fflush(None)
    saved = os.dup(1)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 1)
        try:
            call()
            libc.fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        f.seek(0)
        return f.read().decode()


def entries(B, triples):
    e = np.zeros(len(triples), dtype=B.ENTRY_DTYPE)
    for k, v in enumerate(triples):
        e[k] = v
    return e


SOLVES = {"pcg": lambda B, op, m, pc, b: B.pcg_solve_device(op, m, pc, b, np.zeros(len(b)), verbose=2),
          "bicgstab": lambda B, op, m, pc, b: B.bicgstab_solve(op, m, pc, b, np.zeros(len(b)), verbose=2),
          "gcr": lambda B, op, m, pc, b: B.gcr_solve(op, m, pc, b, np.zeros(len(b)), verbose=2)}
SWAP = [(0, 1, 1.0), (1, 0, 1.0)]      # p.Ap = 0 (PCG), sigma = r^.v = 0 (BiCGSTAB) in iteration 1
QUARTER = [(0, 1, 1.0), (1, 0, -1.0)]  # q = A r is orthogonal to r: rho = r.q = 0 with gamma = 1 (GCR)
BREAKDOWN = {"pcg": SWAP, "bicgstab": SWAP, "gcr": QUARTER}


def printed(B, solver, system):
    """stdout of one verbose = 2 solve, the time values masked. system: "grid" (kind "jacobi"; GCR: "none") or "breakdown"."""
    B.lib().spmv_amd_reset_host_matrices()
    if system == "grid":
        op = B.Operator("stencil5-csr")
        assert op.init_synthetic(8) == 0
        m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), 64, 64, 8)
        pc, b = B.Precond(op, "none" if solver == "gcr" else "jacobi"), np.ones(64)
    else:
        m = B.HostMatrix(entries(B, BREAKDOWN[solver]), 2, 2, -1)
        op = B.Operator("cusparse-csr")
        assert op.init(m) == 0
        pc, b = B.Precond(op, "none"), np.array([1.0, 0.0])
    text = stdout_of(lambda: SOLVES[solver](B, op, m, pc, b))
    pc.destroy()
    op.free()
    return TIMES.sub(r"\g<1>T ms", text)


TAIL = """     Total:      T ms
     SpMV:       T ms
     BLAS1:      T ms
     Reductions: T ms
"""

EXPECTED = {
    ("pcg", "grid"): """[PCG-DEVICE] Initial residual: 8.000000e+00 (preconditioner jacobi)
[PCG-DEVICE] Iter   1: residual = 3.265986e+00 (rel = 4.082483e-01)
[PCG-DEVICE] Iter   2: residual = 1.190826e+00 (rel = 1.488533e-01)
[PCG-DEVICE] Iter   3: residual = 5.180955e-01 (rel = 6.476193e-02)
[PCG-DEVICE] Iter   4: residual = 1.889110e-01 (rel = 2.361387e-02)
[PCG-DEVICE] Iter   5: residual = 5.164515e-02 (rel = 6.455644e-03)
[PCG-DEVICE] Iter   6: residual = 1.080436e-02 (rel = 1.350544e-03)
[PCG-DEVICE] Iter   7: residual = 2.663555e-03 (rel = 3.329443e-04)
[PCG-DEVICE] Iter   8: residual = 3.123303e-04 (rel = 3.904128e-05)
[PCG-DEVICE] Iter   9: residual = 3.226361e-05 (rel = 4.032951e-06)
[PCG-DEVICE] Iter  10: residual = 8.161672e-18 (rel = 1.020209e-18)
[PCG-DEVICE] Converged: YES
[PCG-DEVICE] Iterations: 10
[PCG-DEVICE] Final residual: 8.161672e-18
[PCG-DEVICE] Time breakdown:
""" + TAIL,
    ("pcg", "breakdown"): """[PCG-DEVICE] Initial residual: 1.000000e+00 (preconditioner none)
[PCG-DEVICE] Iter   1: residual = 1.000000e+00 (rel = 1.000000e+00)
[PCG-DEVICE] Breakdown in iteration 1 (pAp or r.z zero or not finite)
[PCG-DEVICE] Converged: NO
[PCG-DEVICE] Iterations: 1
[PCG-DEVICE] Final residual: 1.000000e+00
[PCG-DEVICE] Time breakdown:
""" + TAIL,
    ("bicgstab", "grid"): """[BICGSTAB-DEVICE] Initial residual: 8.000000e+00 (preconditioner jacobi)
[BICGSTAB-DEVICE] Iter   1: residual = 1.170938e+00 (rel = 1.463673e-01)
[BICGSTAB-DEVICE] Iter   2: residual = 2.734238e-01 (rel = 3.417797e-02)
[BICGSTAB-DEVICE] Iter   3: residual = 5.517111e-02 (rel = 6.896389e-03)
[BICGSTAB-DEVICE] Iter   4: residual = 7.563920e-03 (rel = 9.454900e-04)
[BICGSTAB-DEVICE] Iter   5: residual = 5.690096e-04 (rel = 7.112620e-05)
[BICGSTAB-DEVICE] Iter   6: residual = 3.081468e-05 (rel = 3.851836e-06)
[BICGSTAB-DEVICE] Iter   7: residual = 3.896358e-06 (rel = 4.870448e-07)
[BICGSTAB-DEVICE] Converged: YES
[BICGSTAB-DEVICE] Iterations: 7
[BICGSTAB-DEVICE] Final residual: 3.896358e-06
[BICGSTAB-DEVICE] Time breakdown:
""" + TAIL,
    ("bicgstab", "breakdown"): """[BICGSTAB-DEVICE] Initial residual: 1.000000e+00 (preconditioner none)
[BICGSTAB-DEVICE] Iter   1: residual = 1.000000e+00 (rel = 1.000000e+00)
[BICGSTAB-DEVICE] Breakdown in iteration 1 (sigma = r^.v zero or not finite)
[BICGSTAB-DEVICE] Converged: NO
[BICGSTAB-DEVICE] Iterations: 1
[BICGSTAB-DEVICE] Final residual: 1.000000e+00
[BICGSTAB-DEVICE] Time breakdown:
""" + TAIL,
    ("gcr", "grid"): """[GCR-DEVICE] Initial residual: 8.000000e+00 (preconditioner none, restart 16)
[GCR-DEVICE] Iter   1: residual = 3.023716e+00 (rel = 3.779645e-01)
[GCR-DEVICE] Iter   2: residual = 1.107996e+00 (rel = 1.384995e-01)
[GCR-DEVICE] Iter   3: residual = 4.693220e-01 (rel = 5.866525e-02)
[GCR-DEVICE] Iter   4: residual = 1.752468e-01 (rel = 2.190585e-02)
[GCR-DEVICE] Iter   5: residual = 4.953876e-02 (rel = 6.192346e-03)
[GCR-DEVICE] Iter   6: residual = 1.055621e-02 (rel = 1.319526e-03)
[GCR-DEVICE] Iter   7: residual = 2.582611e-03 (rel = 3.228264e-04)
[GCR-DEVICE] Iter   8: residual = 3.100710e-04 (rel = 3.875888e-05)
[GCR-DEVICE] Iter   9: residual = 3.209036e-05 (rel = 4.011295e-06)
[GCR-DEVICE] Iter  10: residual = 7.229271e-16 (rel = 9.036588e-17)
[GCR-DEVICE] Converged: YES
[GCR-DEVICE] Iterations: 10
[GCR-DEVICE] Final residual: 7.229271e-16
[GCR-DEVICE] Time breakdown:
""" + TAIL,
    ("gcr", "breakdown"): """[GCR-DEVICE] Initial residual: 1.000000e+00 (preconditioner none, restart 16)
[GCR-DEVICE] Iter   1: residual = 1.000000e+00 (rel = 1.000000e+00)
[GCR-DEVICE] Breakdown in iteration 1 (rho = r.q zero or not finite)
[GCR-DEVICE] Converged: NO
[GCR-DEVICE] Iterations: 1
[GCR-DEVICE] Final residual: 1.000000e+00
[GCR-DEVICE] Time breakdown:
""" + TAIL,
}


@pytest.mark.parametrize("system", ["grid", "breakdown"])
@pytest.mark.parametrize("solver", ["pcg", "bicgstab", "gcr"])
def test_stdout_line_by_line(B, solver, system):
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    got = printed(B, solver, system)
    print(got)
    assert got.splitlines() == EXPECTED[(solver, system)].splitlines()
