"""GCR(m), CPU side: the new entry points are exported, declared and listed; the argument checks of the solve, of
spmv_amd_gcr_workspace_bytes and of the LAB build's spmv_amd_gcr_stage refuse bad calls before any HIP call (so they hold on a machine
without a GPU); and the INPUTS of the GPU tests are sound: on every row of gcr_restatement.TABLE two roundings of the restatement take
the recorded iteration count and agree within the recorded bound, the bit-exact form agrees with them within the bound of a third
rounding, the recorded residual is the true one (long double), and no history ever grows."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import gcr_restatement as G
from conftest import ROOT
from gcr_restatement import APP_CASE, TABLE, entries_of, hist_err, table_system, third_rounding_bound, true_residual_norm

NEW = ["spmv_amd_gcr_solve_device", "spmv_amd_gcr_last_history", "spmv_amd_gcr_workspace_bytes"]
HOOK = "spmv_amd_gcr_stage"
IDS = [f"{r[0]}-{r[1]}-m{r[2]}-{r[3]:g}" for r in TABLE]
# the rows of the issue: (system, kind, restart) -> iterations at tol 1e-6 / 1e-10
ISSUE_ROWS = 21


def test_gcr_symbols_exported_declared_and_listed(B, Blab):
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
    assert "stagnate" in api.lower()  # api.h says what kind "chebyshev" may do on a nonsymmetric spectrum
    # the binding's mirror of lab.h's constants
    for name, value in (("SPMV_AMD_GCR_MAX_RESTART", B.GCR_MAX_RESTART), ("SPMV_AMD_GCR_DOT_CHUNK", B.GCR_DOT_CHUNK),
                        ("SPMV_AMD_GCR_ORTH_CHUNK", B.GCR_ORTH_CHUNK)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", lab), name
    assert C.sizeof(B.GcrScalars) == 8 * (2 * B.GCR_MAX_RESTART + 4) + 16


def test_the_table_has_the_rows_of_the_issue():
    """At most a quarter of the 21 rows (system, kind, restart) may be missing, and each row is there at both tolerances."""
    rows = {(r[0], r[1], r[2]) for r in TABLE}
    assert len(rows) >= ISSUE_ROWS - ISSUE_ROWS // 4
    for row in rows:
        assert {r[3] for r in TABLE if (r[0], r[1], r[2]) == row} == {1e-6, 1e-10}, row
    assert len(set((r[0], r[1], r[2], r[3]) for r in TABLE)) == len(TABLE)


@pytest.mark.parametrize("row", range(len(TABLE)), ids=IDS)
def test_the_table_holds_in_two_roundings(row):
    """Equal iteration counts -- the table's --, both converged, histories within the stored bound, the converging ratio not a
    rounding error away from tol, the recorded residual the true one (long double) to 1e-6 relative and so below tol, and no
    history that grows."""
    name, kind, restart, tol, iterations, bound = TABLE[row]
    A, b, x0 = table_system(name)
    (x1, h1, i1, c1, e1), (x2, h2, i2, c2, e2) = G.two_roundings(name, kind, restart, tol)
    case = (name, kind, restart, tol)
    assert i1 == i2 == iterations and c1 and c2 and e1 == e2 == "converged", (case, i1, i2, e1, e2)
    err = hist_err(h1, h2)
    print(f"{case}: {i1} iterations, the roundings disagree by {err:.2e} (bound {bound:.0e})")
    assert len(h1) == len(h2) == iterations + 1 and err <= bound, (case, err)
    assert h1[-1] / h1[0] < tol <= h1[-2] / h1[0]
    assert abs(h1[-1] / h1[0] / tol - 1.0) > 1e3 * bound and abs(h1[-2] / h1[0] / tol - 1.0) > 1e3 * bound, case
    e = entries_of(A)
    for x, h in ((x1, h1), (x2, h2)):
        true = true_residual_norm(e, b, x)
        assert abs(true - h[-1]) <= 1e-6 * h[-1] and true < tol * h[0], (case, true, h[-1])
        assert np.max(np.diff(h)) <= 1e-12 * h[0], case  # minimal residual: never grows
    _, h0, _, _, _ = G.gcr(A, b, np.zeros_like(b), G.make_apply(A, G.dimension_of(name), kind), restart, tol, 0)
    assert abs(h0[0] - h1[0]) > 1e-3 * h1[0], case  # x0 matters to the first residual


def exact_row(O, name, kind, restart, tol, max_iters=1000):
    A, b, x0 = table_system(name)
    dim = G.dimension_of(name)
    rp, ci, va = O.build_csr(entries_of(A), A.shape[0])
    grid = G.grid_of(A, dim)
    matvec = (lambda u: O.spmv_csr(rp, ci, va, u)) if dim == 3 else (lambda u: O.spmv_stencil5(rp, ci, va, u, grid))
    return G.gcr_exact(matvec, b, x0, G.exact_apply(O, A, dim, kind), restart, tol, max_iters)


@pytest.mark.parametrize("row", range(len(TABLE)), ids=IDS)
def test_the_exact_form_agrees_with_plain_numpy(O, row):
    """gcr_exact -- the product and the application in the operator's bits, the dots as the kernels sum them, every update an fma --
    is a third rounding of the same algebra: the table's count, history and x within the row's bound for a third rounding -- what the
    device, which equals this form bit for bit, is held to against plain numpy."""
    name, kind, restart, tol, iterations, stored = TABLE[row]
    bound = third_rounding_bound(stored)
    A, b, x0 = table_system(name)
    (x1, h1, _, _, _), _ = G.two_roundings(name, kind, restart, tol)
    x, h, it, conv, how = exact_row(O, name, kind, restart, tol)
    assert it == iterations and conv and how == "converged", (it, how)
    err = hist_err(h, h1)
    print(f"{(name, kind, restart, tol)}: exact against plain {err:.2e} (bound {bound:.0e})")
    assert err <= bound and np.max(np.abs(x - x1)) <= bound * np.max(np.abs(x1))
    true = true_residual_norm(entries_of(A), b, x)
    assert abs(true - h[-1]) <= 1e-6 * h[-1] and true < tol * h[0]
    assert np.max(np.diff(h)) <= 1e-12 * h[0]


def test_jacobi_counts_equal_none_counts_on_constant_diagonals():
    """On a constant diagonal Jacobi scales z and q by one number, which GCR's alpha undoes: the same iterates."""
    for name in ("grid33", "cube16"):
        A, b, x0 = table_system(name)
        dim = G.dimension_of(name)
        for restart in (4, 16):
            for tol in (1e-6, 1e-10):
                want = [r[4] for r in TABLE if r[:4] == (name, "none", restart, tol)]
                if not want:
                    continue
                x, h, it, conv, _ = G.gcr(A, b, x0, G.make_apply(A, dim, "jacobi"), restart, tol)
                assert conv and it == want[0], (name, restart, tol, it, want)


def test_a_restart_that_never_fills_and_restart_one_run_the_loop(O):
    """m >= iterations: one basis for the whole solve (full GCR), the count no larger than any restarted one's; m = 1: no basis is
    ever read (steepest descent on the residual), still convergent and monotone. Both in plain numpy and in the exact form; restart 0
    is restart 16."""
    name, kind, tol = "grid33", "multigrid1", 1e-6
    A, b, x0 = table_system(name)
    runs = {}
    for restart in (1, 4, 32):
        plain = G.gcr(A, b, x0, G.make_apply(A, 2, kind), restart, tol)
        exact = exact_row(O, name, kind, restart, tol)
        assert plain[3] and exact[3] and plain[2] == exact[2], (restart, plain[2:], exact[2:])
        assert hist_err(exact[1], plain[1]) <= 1e-10
        assert np.max(np.diff(plain[1])) <= 1e-12 * plain[1][0]
        runs[restart] = plain[2]
    assert runs[32] < 32 and runs[32] <= runs[4] <= runs[1], runs
    a = G.gcr(A, b, x0, G.make_apply(A, 2, kind), 0, tol)
    c = G.gcr(A, b, x0, G.make_apply(A, 2, kind), 16, tol)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    # max_iters inside a basis: the count is max_iters, not converged
    x, h, it, conv, end = G.gcr(A, b, x0, G.make_apply(A, 2, kind), 4, tol, 3)
    assert (it, conv, end) == (3, False, "max_iters") and len(h) == 4


def test_the_application_case_holds_in_every_rounding(O):
    """b = 1, x0 = 0 on the 33 grid (what apps/cg_solver solves on the written file): APP_CASE's count in the two CPU roundings and in
    the exact form, and the converging ratio far from tol."""
    n, restart, kind, iterations = APP_CASE
    A = G.convdiff5(n)
    b, x0 = np.ones(n * n), np.zeros(n * n)
    rp, ci, va = O.build_csr(entries_of(A), n * n)
    runs = [G.gcr(A, b, x0, G.make_apply(A, 2, kind), restart), G.gcr_other_rounding(A, b, x0, G.make_apply(A, 2, kind, csc=True), restart),
            G.gcr_exact(lambda u: O.spmv_stencil5(rp, ci, va, u, n), b, x0, G.exact_apply(O, A, 2, kind), restart)]
    assert all(r[2] == iterations and r[3] for r in runs), [r[2:] for r in runs]
    h = runs[0][1]
    assert h[-1] / h[0] < 0.96e-6 and h[-2] / h[0] > 3e-6


def test_breakdowns_in_the_restatement(O):
    """A = 0 I (stored zeros): q = 0, gamma = 0 -- iteration 1 is counted, the unchanged residual recorded, x = x0 bit for bit. A
    rotation by a quarter turn: q is orthogonal to r, rho = 0 with gamma = 1 -- the same ending named "rho". Both in every form."""
    b, x0 = np.array([1.5, -0.75, 2.0]), np.array([0.25, 0.5, -1.0])
    zero = sp.csr_matrix((np.zeros(3), (np.arange(3), np.arange(3))), shape=(3, 3))
    turn = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    for A, bb, xx, want in ((zero, b, x0, "gamma"), (turn, np.array([1.0, 0.0]), np.zeros(2), "rho")):
        n = A.shape[0]
        e = np.zeros(A.nnz, dtype=entries_of(sp.identity(2)).dtype)
        c = sp.coo_matrix(A)
        e["row"], e["col"], e["value"] = c.row, c.col, c.data
        rp, ci, va = O.build_csr(e, n)
        for run in (G.gcr(A, bb, xx, lambda r: r, 4), G.gcr_other_rounding(A, bb, xx, lambda r: r, 4),
                    G.gcr_exact(lambda u: O.spmv_csr(rp, ci, va, u), bb, xx, lambda r: 2.0 * r, 4)):
            x, h, it, conv, end = run
            assert (it, conv, end) == (1, False, want) and np.array_equal(x, xx) and len(h) == 2 and h[1] == h[0] > 0.0, run


def _free_all(B):
    # free() of an operator that was never initialised touches no device memory: safe without a GPU, and it makes "used before
    # init" hold even when GPU tests ran earlier in the same process
    for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
        B.Operator(mode).free()


def test_gcr_solve_refuses_without_touching_the_gpu(B, capfd):
    _free_all(B)
    L = B._gcr_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    b, x = np.ones(n), np.zeros(n)
    cfg, st = B.CGConfig(10, 1e-6, 0, 0), B.CGStats()
    fake = C.c_void_p(16)  # never dereferenced: every call it is given to is refused before the preconditioner is looked at

    def refused(op, pm=None, mat=m.ptr, restart=4, bb=b.ctypes.data, xx=x.ctypes.data, c=C.byref(cfg), s=C.byref(st), word="[GCR]"):
        rc = L.spmv_amd_gcr_solve_device(op, mat, pm, restart, bb, xx, c, s)
        err = capfd.readouterr().err
        assert rc != 0 and "[GCR]" in err and word in err and err.count("\n") == 1, (rc, err)

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
    for restart in (-1, 33, 1 << 20):
        refused(stencil, fake, restart=restart, word=f"restart = {restart}")
    assert np.all(x == 0.0)
    assert L.spmv_amd_gcr_last_history(None, 0) >= 0
    L.spmv_amd_pcg_release_workspace()                      # nothing held: a no-op


def test_gcr_solve_refuses_what_needs_a_preconditioner_record(B, capfd):
    """The first two ints of SpmvAmdPrecond are kind and n (csrc/precond.hpp). A record of a kind this library does not make is
    refused as foreign; every operator of the library used before init is refused before the pair is looked at, for EVERY kind (none
    is turned away for being "chebyshev" or "multigrid"); a caller's operator table has its sizes checked against the record."""
    _free_all(B)
    L = B._gcr_lib()
    n = 9
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n, n, 3)
    b, x = np.ones(n), np.zeros(n)
    cfg, st = B.CGConfig(10, 1e-6, 0, 0), B.CGStats()

    def solve(op, record, mat=m):
        rc = L.spmv_amd_gcr_solve_device(op, mat.ptr, C.cast(record, C.c_void_p), 0, b.ctypes.data, x.ctypes.data, C.byref(cfg), C.byref(st))
        return rc, capfd.readouterr().err

    for kind in (-1, 4, 7):
        record = (C.c_int * 256)()
        record[0], record[1] = kind, n
        rc, err = solve(B.Operator("stencil5-csr").op, record)
        assert rc != 0 and "[GCR]" in err and "not one of this library's" in err and "refused" in err, err
    for kind in (0, 1, 2, 3):
        record = (C.c_int * 256)()
        record[0], record[1] = kind, n
        for mode in ("stencil5-csr", "stencil7-csr", "cusparse-csr", "ellpack", "stencil5-ellpack"):
            rc, err = solve(B.Operator(mode).op, record)
            assert rc != 0 and "used before init" in err and "[GCR]" in err and "symmetric" not in err, (mode, err)
    own = B.SpmvOperator()
    own.name = b"mine"
    own.run_device = B.RUN_DEVICE_FN(lambda dx, dy: 1)  # never called
    record = (C.c_int * 256)()
    record[0], record[1] = 1, n - 1
    rc, err = solve(C.pointer(own), record)
    assert rc != 0 and "[GCR]" in err and f"the preconditioner is for {n - 1} rows, mat->rows = {n}" in err, err
    empty = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), 0, 0, -1)
    rc, err = solve(C.pointer(own), record, empty)
    assert rc != 0 and "[GCR]" in err and "mat->rows < 1" in err, err
    assert np.all(x == 0.0)


def test_gcr_workspace_bytes(B):
    """0 for refused arguments; else x, b, r, 2 m basis vectors, the partials and the kind's scratch: exactly 2 * 8 * rows more per
    unit of restart, one vector more for "jacobi", three for "chebyshev", none for "multigrid"; restart 0 is restart 16."""
    W = B.gcr_workspace_bytes
    for rows, restart, kind in ((0, 4, "none"), (-5, 4, "none"), (100, -1, "none"), (100, 33, "none"), (100, 4, None), (100, 4, ""),
                                (100, 4, "ilu0"), (100, 4, "Jacobi"), (100, 4, "multigrid3d")):
        assert W(rows, restart, kind) == 0, (rows, restart, kind)
    for rows in (1, 2, 127, 4225, 20000 * 20000):
        count = max(1, ((rows >> 1) + 63) // 64)
        for kind, extra in (("none", 0), ("jacobi", 1), ("chebyshev", 3), ("multigrid", 0)):
            sizes = [W(rows, m, kind) for m in range(1, 33)]
            assert all(b - a == 2 * 8 * rows for a, b in zip(sizes, sizes[1:])), (rows, kind)
            assert sizes[0] == (3 + 2 + extra) * 8 * rows + 32 * 8 * count, (rows, kind, sizes[0])
            assert W(rows, 0, kind) == sizes[15]


def test_gcr_stage_refuses_without_touching_the_gpu(Blab, capfd):
    """spmv_amd_gcr_stage (LAB build, include/spmv_amd/lab.h): an unknown stage or kind, null arguments, n < 1, a slot outside the
    stage's range, count < 1, a null or misaligned pointer the stage needs -- each refused before any HIP call, non-zero, with a
    sentence on stderr. The pointers are never dereferenced."""
    good, odd, crooked = 4096, 4096 + 8, 4096 + 4  # 16-byte aligned; 8-byte aligned only; not even that

    def basis(**kw):
        arr = (C.c_void_p * 32)(*([good] * 32))
        for i, v in kw.items():
            arr[int(i[1:])] = v
        return arr

    def args(**kw):
        a = Blab.GcrStageArgs(n=5, b=good, v=good, dinv=good, x=good, r=good, zs=good, z_in=good, Q=basis(), Z=basis(), slot=2,
                              partials=good, count=3, which=3, tol=1e-6, hist=good, hist_cap=4)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(stage, kind, a, sc, word):
        rc = Blab.gcr_stage(stage, kind, a, sc)
        err = capfd.readouterr().err
        assert rc != 0 and "[GCR]" in err and "refused" in err and word in err, (stage, kind, word, rc, err)

    sc = Blab.GcrScalars()
    for stage in (None, "", "Init", "update", "dot", "orthogonalize", "update_r"):
        refused(stage, "jacobi", args(), sc, "stage")
    needs = {"init": ("b", "v", "r", "dinv", "zs"), "multidot": (), "orthogonalise": ("z_in", "r"), "update_xr": ("x", "r", "dinv", "zs")}
    for stage, vectors in needs.items():
        refused(stage, "jacobi", None, sc, "null arguments")
        if stage in ("init", "update_xr"):
            for kind in (None, "", "ilu0", "Jacobi", "chebyshev", "multigrid"):
                refused(stage, kind, args(), sc, "kind")
        refused(stage, "jacobi", args(n=0), sc, "n < 1")
        for name in vectors:
            for kind in ("jacobi", "none"):
                if kind == "none" and name in ("dinv", "zs"):
                    continue  # not looked at
                refused(stage, kind, args(**{name: None}), sc, name + " is null")
                refused(stage, kind, args(**{name: odd}), sc, name + " is not 16-byte aligned")
        refused(stage, "none", args(partials=None), sc, "partials is null")
        refused(stage, "none", args(partials=crooked), sc, "partials is not 8-byte aligned")
        if stage != "init":
            refused(stage, "none", args(), None, "scalar record")
            refused(stage, "none", args(slot=32), sc, "slot")
            refused(stage, "none", args(slot=-1), sc, "slot")
            refused(stage, "none", args(Q=None), sc, "Q is null")
            refused(stage, "none", args(Q=basis(q2=None)), sc, "Q[2] is null")
            refused(stage, "none", args(Q=basis(q2=odd)), sc, "Q[2] is not 16-byte aligned")
            # slots past `slot` are not looked at: refused for another reason
            refused(stage, "none", args(Q=basis(q3=None, q31=odd), partials=None), sc, "partials is null")
    refused("multidot", None, args(slot=0), sc, "slot")
    refused("multidot", None, args(Q=basis(q0=None)), sc, "Q[0] is null")
    refused("orthogonalise", None, args(Z=None), sc, "Z is null")
    refused("orthogonalise", None, args(Z=basis(z1=odd)), sc, "Z[1] is not 16-byte aligned")
    refused("update_xr", "none", args(Z=basis(z2=None)), sc, "Z[2] is null")
    refused("reduce", None, None, sc, "null arguments")
    refused("reduce", None, args(), None, "scalar record")
    for count in (0, -1):
        refused("reduce", None, args(count=count), sc, "count < 1")
    for which in (-1, 4):
        refused("reduce", None, args(which=which), sc, "which")
    refused("reduce", None, args(which=1, slot=0), sc, "slot")
    refused("reduce", None, args(which=1, slot=32), sc, "slot")
    refused("reduce", None, args(hist_cap=-1), sc, "hist_cap")
    refused("reduce", None, args(partials=None), sc, "partials is null")
    refused("reduce", None, args(partials=crooked), sc, "partials is not 8-byte aligned")
    refused("reduce", None, args(hist=None), sc, "hist is null")
    refused("reduce", None, args(hist=crooked), sc, "hist is not 8-byte aligned")
    with pytest.raises(RuntimeError):  # the product library has no such entry point
        __import__("conftest").load_binding().gcr_stage("reduce", None, args(), sc)
