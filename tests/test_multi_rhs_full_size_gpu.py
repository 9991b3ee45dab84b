"""The batched CG at the benchmark's full size: 20 000^2 (4 x 10^8 unknowns), four columns, through the stencil5-csr operator
generated in HBM. Column 0 (b = 1) is the published system: 14 iterations, the committed golden history and checksums. Column 1
(b = 2) is exactly twice column 0."""
import numpy as np
import pytest

from conftest import hist_err

pytestmark = pytest.mark.gpu


def test_cg_multi_20k_four_columns_golden_and_exact_scaling(B, golden):
    g = golden["cases"].get("20000:5.0")
    if g is None:
        pytest.skip("20k golden not generated")
    g = g["cg"]
    n = 20000
    N = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    shell = B.HostMatrix(np.empty(0, dtype=B.ENTRY_DTYPE), N, N, n)  # the solver reads mat->rows only
    Bk = np.empty((4, N))
    Bk[0] = 1.0
    Bk[1] = 2.0
    Bk[2] = 1.25
    Bk[2] += 0.01 * np.sin(np.arange(N, dtype=np.float64) * 1e-3)
    Bk[3] = 1.5
    X, hists, stats = B.cg_solve_multi(op, shell, Bk, np.zeros((4, N)))
    del Bk
    s0 = stats[0]
    assert s0.iterations == g["iterations"] == 14 and s0.converged == 1
    assert hist_err(hists[0], g["history"]) < 1e-10
    assert abs(s0.solution_sum - g["solution_sum"]) <= 1e-10 * abs(g["solution_sum"])
    assert abs(s0.solution_norm - g["solution_norm"]) <= 1e-10 * g["solution_norm"]
    assert np.array_equal(hists[1], 2.0 * hists[0]) and np.array_equal(X[1], 2.0 * X[0])
    assert stats[1].iterations == 14 and stats[1].solution_sum == 2.0 * s0.solution_sum
    for j in (2, 3):
        assert stats[j].converged == 1 and hists[j][-1] / hists[j][0] < 1e-6
    op.free()
