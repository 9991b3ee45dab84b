"""The Chebyshev polynomial preconditioner, CPU side: the three new entry points are declared, exported and bound; every refusal that
needs no device returns NULL or non-zero before any HIP call (so it holds on a machine without a GPU); the restatement the GPU tests
compare against takes the table's iteration counts in two independent roundings, which agree far below the 1e-10 the GPU is held to;
and the symmetric Gershgorin bound is a bound (against scipy's eigsh) with the value the algebra says."""
import ctypes as C
import math
import os
import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import chebyshev_restatement as R
import pcg_restatement as P
from conftest import ROOT

NEW = ["spmv_amd_precond_create_chebyshev", "spmv_amd_precond_chebyshev_info", "spmv_amd_precond_apply_device"]
OPERATORS = ("stencil5-csr", "cusparse-csr", "ellpack", "stencil5-ellpack")


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


def test_chebyshev_symbols_exported_declared_and_bound(B):
    L = B._pcg_lib()
    api = open(os.path.join(ROOT, "include", "spmv_amd", "api.h")).read()
    exports = open(os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", api), name
        assert re.search(r"^\s+" + name + r";", exports, flags=re.M), name
        assert name in B.DECLARED_SYMBOLS and name not in B.LAB_ONLY_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for method in ("chebyshev", "chebyshev_info", "apply_device"):
        assert callable(getattr(B.Precond, method)), method
    assert "spmv_amd_pcg_last_step_launches" in B.LAB_ONLY_SYMBOLS and not hasattr(B.lib(), "spmv_amd_pcg_last_step_launches")


def test_chebyshev_refuses_without_touching_the_gpu(B):
    for mode in OPERATORS:  # free() of an operator that was never initialised touches no device memory
        B.Operator(mode).free()
    L = B._pcg_lib()
    bad = C.c_int(7)
    stencil = B.Operator("stencil5-csr").op
    nan, inf = float("nan"), float("inf")

    def refused(op, degree, lo, hi, bad_row=bad):
        bad.value = 7
        got = L.spmv_amd_precond_create_chebyshev(op, degree, lo, hi, None if bad_row is None else C.byref(bad_row))
        return not got and (bad_row is None or bad.value == -1)

    assert refused(None, 4, 0.0, 0.0)
    for degree in (-1, 33, -2 ** 31, 2 ** 31 - 1):
        assert refused(stencil, degree, 0.0, 0.0), degree
    for lo, hi in ((2.0, 2.0), (3.0, 2.0), (nan, 2.0), (0.1, nan), (nan, nan), (0.0, nan), (nan, 0.0), (0.1, inf), (inf, inf), (-inf, 2.0)):
        assert refused(stencil, 4, lo, hi), (lo, hi)
    for mode in OPERATORS:  # used before init: with and without explicit bounds, every degree at the ends of the range
        for degree, lo, hi in ((0, 0.0, 0.0), (4, 0.1, 2.0), (32, 0.0, 2.0)):
            assert refused(B.Operator(mode).op, degree, lo, hi), mode
    assert refused(stencil, 4, 0.1, 2.0, bad_row=None)            # bad_row may be NULL
    own = B.SpmvOperator()                                        # a caller's own table: no matrix to read
    own.name = b"mine"
    assert refused(C.pointer(own), 4, 0.1, 2.0)

    deg, lo, hi = C.c_int(-5), C.c_double(-5.0), C.c_double(-5.0)
    coef = np.full(3, -5.0)
    assert L.spmv_amd_precond_chebyshev_info(None, C.byref(deg), C.byref(lo), C.byref(hi), coef.ctypes.data, 3) == 0
    assert (deg.value, lo.value, hi.value) == (-5, -5.0, -5.0) and np.all(coef == -5.0)  # nothing written

    good = C.c_void_p(4096)  # never dereferenced
    rz = C.c_double(-5.0)
    for op, m, r, z in ((None, good, good, good), (stencil, None, good, good), (stencil, good, None, good), (stencil, good, good, None)):
        assert L.spmv_amd_precond_apply_device(op, m, r, z, C.byref(rz)) != 0
    for r, z in ((4096 + 8, 8192), (4096, 8192 + 8)):              # a misaligned vector is refused before m is looked at
        assert L.spmv_amd_precond_apply_device(stencil, good, C.c_void_p(r), C.c_void_p(z), None) != 0
    assert rz.value == -5.0


def test_coefficients_are_the_chebyshev_polynomial():
    """The recurrence, restated independently: after k steps of the application the error polynomial 1 - lambda q_k(lambda) is
    T_k((theta - lambda) / delta) / T_k(theta / delta), whatever r is. Checked on a diagonal B with eigenvalues across and
    outside the interval."""
    lo, hi = 0.07, 1.9
    lam = np.linspace(0.01, 2.2, 400)
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    for degree in (0, 1, 2, 5, 8):
        coef = R.coefficients(degree, lo, hi)
        assert len(coef) == 1 + 2 * degree
        z = R.make_apply(lambda v: lam * v, np.ones_like(lam), coef)(np.ones_like(lam))  # z = q(lambda)
        cheb = np.polynomial.chebyshev.Chebyshev.basis(degree + 1)
        want = cheb((theta - lam) / delta) / cheb(theta / delta)
        assert np.max(np.abs((1.0 - lam * z) - want)) < 1e-12, degree


def test_gershgorin_bound_is_a_bound_with_the_value_the_algebra_gives():
    """>= eigsh's largest eigenvalue of D^-1/2 A D^-1/2; 1.8 on the centre-5 stencils however they are scaled (the plain row sum of
    D^-1 A gives 61.8 on scaled127), 2.0 on the Poisson stencil, to 4 ulp."""
    for name, value in (("scaled127", 1.8), ("negated65", 1.8), ("poisson64", 2.0), ("plain127", 1.8), ("scaled601", 1.8)):
        A, _, _ = R.table_system(name)
        d = P.diagonal(A)
        bound = R.gershgorin(A, 1.0 / d)
        assert ulps(bound, value) <= 4, (name, bound)
        if name in ("scaled127", "negated65", "poisson64"):
            s = sp.diags(1.0 / np.sqrt(np.abs(d)))
            top = float(sla.eigsh(sp.csr_matrix(np.sign(d[0]) * (s @ A @ s)), k=1, which="LA", return_eigenvectors=False)[0])
            assert 0.9 * value < top <= bound, (name, top, bound)
    A, _, _ = R.table_system("scaled127")
    plain = float(np.max(np.asarray(abs(sp.diags(1.0 / P.diagonal(A)) @ A).sum(axis=1))))
    assert plain > 30.0  # what the symmetric form is for
    lo, hi = R.interval(A, 1.0 / P.diagonal(A))
    assert hi == R.gershgorin(A, 1.0 / P.diagonal(A)) and lo == hi / 30.0
    assert R.interval(A, None, 0.25, 3.0) == (0.25, 3.0)


def test_the_chebyshev_table_holds_in_two_roundings():
    """Every row of the table (without the 640^2 ones, minutes on a CPU): the iteration count it records in the restatement and in
    its other rounding, histories within 1e-12 (measured 1e-15 .. 1.3e-14) and x within 1e-11: 1e-10 against the restatement is a
    property of these inputs, not of a summation order. Jacobi rows pin the counts the polynomial is compared with."""
    systems = {}
    for name, degree, tol, iterations in R.TABLE:
        if name in R.HOST_SKIPS:
            continue
        if name not in systems:
            A, b, x0 = R.table_system(name)
            dinv = 1.0 / P.diagonal(A)
            systems[name] = (A, b, x0, dinv, R.interval(A, dinv))
        A, b, x0, dinv, (lo, hi) = systems[name]
        case = (name, degree, tol)
        if degree is None:
            _, h, it, conv = P.pcg(A, b, x0, dinv, tol, 1000)
            assert conv and it == iterations, (case, it)
            continue
        x1, h1, i1, c1 = R.pcg(A, b, x0, degree, lo, hi, tol, 1000)
        x2, h2, i2, c2 = R.pcg_other_rounding(A, b, x0, degree, lo, hi, tol, 1000)
        err = P.hist_err(h1, h2)
        print(case, i1, i2, f"history {err:.2e}, x {np.max(np.abs(x1 - x2)) / np.max(np.abs(x1)):.2e}")
        assert c1 and c2 and i1 == i2 == iterations, (case, i1, i2)
        assert len(h1) == iterations + 1 and err < 1e-12, (case, err)
        assert np.max(np.abs(x1 - x2)) <= 1e-11 * np.max(np.abs(x1)), case
        # the converging ratio is not a rounding error away from tol
        assert abs(h1[-1] / h1[0] / tol - 1.0) > 1e-6 and abs(h1[-2] / h1[0] / tol - 1.0) > 1e-6, case


def test_degree_zero_is_jacobi_up_to_a_scale():
    """z = c0 dinv r: the same iterates as Jacobi-PCG (the scale cancels in alpha and beta)."""
    A, b, x0 = R.table_system("scaled127")
    dinv = 1.0 / P.diagonal(A)
    lo, hi = R.interval(A, dinv)
    _, hj, ij, _ = P.pcg(A, b, x0, dinv, 1e-6, 1000)
    _, hc, ic, _ = R.pcg(A, b, x0, 0, lo, hi, 1e-6, 1000)
    assert ij == ic and P.hist_err(hc, hj) < 1e-12
