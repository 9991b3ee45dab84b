"""Batched GCR(m) measured against k single-RHS solves (spmv_amd_gcr_solve_device_multi). A tool, not a test.
   python tools/gcr_multi_bench.py [--upwind 2000] [--cube 0] [--ks 1,2,4,8] [--kinds multigrid,jacobi] [--solves 3] [--out FILE]
   python tools/gcr_multi_bench.py --headline 20000 [--k 4] [--restart 4] [--iterations 16] [--solves 5] [--out FILE]
   python tools/gcr_multi_bench.py --stages 15 [--grid 2000] [--k 4] [--calls 7] [--out FILE]
Always against k spmv_amd_gcr_solve_device solves IN THE SAME PROCESS, batched and single alternated (hipMalloc's placement decides a
few percent per process), 1 warm-up + --solves timed rounds, time_total_ms of the batch against the sum of the k
singles' (upload and download are outside both); medians with ranges, the ratio single / batched with its pairwise range.
1. Time to solution on the --upwind grid of tools/gcr_bench.py's 5-point upwind convection-diffusion stencil (px = 2, py = 0.5, shift
   0) and on its --cube 7-point twin, b_j = standard_normal(seed 1 + j), x0 = 0, tol 1e-8, GCR(16), kinds "multigrid" (nu = 1, the
   block hierarchy against the single-vector one) and "jacobi". The batch runs until its last column stops; the singles each their own
   count. Reported with the iteration counts and the true relative residual of every column of the batch.
2. --headline N: the synthetic stencil5-csr grid (+5 / -1), kind "none", a fixed number of whole iterations under a tolerance that is
   never met: ms per system and iteration beside the byte model per row and column, mean over a cycle of m slots: single 128 at
   slot 0 and 144 + 24 j behind it; batched the same less 40 (1 - 1 / k).
3. --stages J (LAB build): the batched multidot and orthogonalise kernels at slot J and the x / r kernel on --grid^2 rows x --k
   columns through spmv_amd_gcr_multi_stage, --calls timed calls each after one warm-up (host clock around the synchronising call);
   the bytes each moves per row and column (multidot 8 (J + 1), orthogonalise 32 + 16 J, x / r 48) over the median time.
Prints one line per measurement and a JSON summary; --out FILE gets both."""
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


upwind_n = opt("--upwind", 2000)
cube_n = opt("--cube", 0)
headline_n = opt("--headline", 0)
stage_slot = opt("--stages", -1)
ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]
kinds = opt("--kinds", "multigrid,jacobi").split(",")
solves = opt("--solves", 3 if headline_n == 0 else 5)
out_path = opt("--out", "")
lines = []
result = {}


def say(text):
    print(text, flush=True)
    lines.append(text)


def finish():
    say(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def cycle_mean(m, k=None):
    """Bytes per row, column and iteration, kind "none", the mean over slots 0 .. m - 1; k: batched, None: the single solver."""
    shared = 0.0 if k is None else 40.0 * (1.0 - 1.0 / k)
    return float(np.mean([(128.0 if j == 0 else 144.0 + 24.0 * j) - shared for j in range(m)]))


# ---- 3. the kernels alone ----
if stage_slot >= 0:
    L = B.use_lab()
    L.require_gpu()
    L.lib().spmv_amd_set_device(0)
    j, k, grid, calls = stage_slot, opt("--k", 4), opt("--grid", 2000), opt("--calls", 7)
    assert 1 <= j < L.GCR_MAX_RESTART and 1 <= k <= 8
    N = grid * grid
    vectors = [L.DeviceVector(N * k, 1.0 / (i + 1)) for i in range(2 * (j + 1) + 2)]
    Q = (C.c_void_p * L.GCR_MAX_RESTART)(*([v.ptr for v in vectors[:j + 1]] + [None] * (L.GCR_MAX_RESTART - j - 1)))
    Z = (C.c_void_p * L.GCR_MAX_RESTART)(*([v.ptr for v in vectors[j + 1:2 * (j + 1)]] + [None] * (L.GCR_MAX_RESTART - j - 1)))
    x, r = vectors[-2], vectors[-1]
    count = (N + 255) // 256
    partials = L.DeviceVector(L.GCR_MAX_RESTART * k * count, 0.0)
    cols = (L.GcrMultiColumn * k)()
    for c in cols:
        c.alpha = 1e-3
        for i in range(j):
            c.beta[i] = 1e-3
    host = np.frombuffer(bytes(cols), dtype=np.float64).copy()
    dcols = L.DeviceVector.from_host(host)
    a = L.GcrMultiStageArgs(n=N, X=x.ptr, R=r.ptr, z_in=r.ptr, Q=Q, Z=Z, slot=j, cols=dcols.ptr, partials=partials.ptr)
    bytes_of = {"multidot": 8 * (j + 1), "orthogonalise": 32 + 16 * j, "update_xr": 48}
    result = {"slot": j, "k": k, "grid": grid, "calls": calls, "stages": {}}
    for stage in ("multidot", "orthogonalise", "update_xr"):
        assert L.gcr_multi_stage(stage, "none", k, a) == 0  # warm-up
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            assert L.gcr_multi_stage(stage, "none", k, a) == 0
            ms.append((time.perf_counter() - t0) * 1e3)
        rate = bytes_of[stage] * N * k / (np.median(ms) * 1e-3) / 1e12
        result["stages"][stage] = dict(spread(ms), bytes_per_row_and_column=bytes_of[stage], tb_per_s=rate)
        say(f"slot {j}, {grid}^2 rows x {k} columns, {stage:13s} {bytes_of[stage]:4d} B per row and column: ms median={np.median(ms):.3f} "
            f"range={min(ms):.3f}..{max(ms):.3f} = {rate:.2f} TB/s")
    xr = result["stages"]["update_xr"]["tb_per_s"]
    for stage in ("multidot", "orthogonalise"):
        say(f"{stage} stream rate / x-r kernel's: {result['stages'][stage]['tb_per_s'] / xr:.3f}")
    for v in vectors + [partials, dcols]:
        v.free()
    finish()

B.require_gpu()
B.lib().spmv_amd_set_device(0)


def alternate(batched, singles):
    """1 warm-up, then --solves rounds of one batched solve and the k singles; ms each."""
    batched(), singles()
    tb, ts = [], []
    for _ in range(solves):
        tb.append(batched())
        ts.append(singles())
    pair = [s / b for s, b in zip(ts, tb)]
    return tb, ts, {"median": float(np.median(ts) / np.median(tb)), "min": min(pair), "max": max(pair)}


# ---- 2. the bare loop on the headline grid ----
if headline_n > 0:
    n, k, m, iterations = headline_n, opt("--k", 4), opt("--restart", 4), opt("--iterations", 16)
    N = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    mat = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)
    pc = B.Precond(op, "none")
    wiggle = 0.01 * np.sin(1e-3 * np.arange(N, dtype=np.float64))
    Bk, X0 = np.stack([(1.0 + j / 8.0) + wiggle for j in range(k)]), np.zeros((k, N))

    def batched():
        _, hists, stats = B.gcr_solve_multi(op, mat, pc, Bk, X0, restart=m, tol=1e-300, max_iters=iterations)
        assert all(s.iterations == iterations for s in stats) and all(np.all(np.isfinite(h)) for h in hists)
        return stats[0].time_total_ms / (iterations * k)

    def singles():
        total = 0.0
        for j in range(k):
            _, h, st = B.gcr_solve(op, mat, pc, Bk[j], X0[j], restart=m, tol=1e-300, max_iters=iterations)
            assert st.iterations == iterations and np.all(np.isfinite(h))
            total += st.time_total_ms
        return total / (iterations * k)

    tb, ts, ratio = alternate(batched, singles)
    model = cycle_mean(m) / cycle_mean(m, k)
    verdict = "met" if ratio["median"] >= model else "missed"
    result = {"headline": {"n": n, "k": k, "restart": m, "iterations": iterations, "operator": op.variant(), "spmm": op.spmm_variant(),
                           "batched_ms_per_system_iteration": spread(tb), "single_ms_per_system_iteration": spread(ts),
                           "single_over_batched": ratio, "model": model, "verdict": verdict}}
    say(f"grid {n}^2, {op.variant()} / {op.spmm_variant()}, kind none, GCR({m}), k={k}, {iterations} iterations: ms per system and iteration batched "
        f"{np.median(tb):.4f} ({min(tb):.4f}..{max(tb):.4f}) = {cycle_mean(m, k) * N / np.median(tb) / 1e9:.2f} TB/s of the model's "
        f"{cycle_mean(m, k):.0f} B, single {np.median(ts):.4f} ({min(ts):.4f}..{max(ts):.4f}) = {cycle_mean(m) * N / np.median(ts) / 1e9:.2f} TB/s "
        f"of {cycle_mean(m):.0f} B; single / batched {ratio['median']:.3f} (pairwise {ratio['min']:.3f}..{ratio['max']:.3f}; model {model:.2f}: "
        f"{verdict}, measured / model {ratio['median'] / model:.3f})")
    pc.destroy()
    op.free()
    finish()


# ---- 1. time to solution on the upwind stencils ----
def upwind(dim, g):
    import scipy.sparse as sp

    px, py, pz, shift = 2.0, 0.5, 1.0, 0.0
    eye = sp.identity(g)
    lower = lambda p: sp.diags([np.full(g - 1, -1.0 - p), np.full(g - 1, -1.0)], [-1, 1])
    if dim == 2:
        t = sp.diags([np.full(g - 1, -1.0 - px), np.full(g, 4.0 + px + py + shift), np.full(g - 1, -1.0)], [-1, 0, 1])
        A = sp.csr_matrix(sp.kron(eye, t) + sp.kron(lower(py), eye))
    else:
        t = sp.diags([np.full(g - 1, -1.0 - px), np.full(g, 6.0 + px + py + pz + shift), np.full(g - 1, -1.0)], [-1, 0, 1])
        A = sp.csr_matrix(sp.kron(eye, sp.kron(eye, t)) + sp.kron(eye, sp.kron(lower(py), eye)) + sp.kron(lower(pz), sp.kron(eye, eye)))
    rows = A.shape[0]
    c = sp.coo_matrix(A)
    pick = np.lexsort((c.col, c.row))
    e = np.zeros(c.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = c.row[pick], c.col[pick], c.data[pick]
    B.lib().spmv_amd_reset_host_matrices()
    mat = B.HostMatrix(e, rows, rows, g)
    op = B.Operator("stencil5-csr" if dim == 2 else "stencil7-csr")
    assert op.init(mat) == 0
    kmax = max(ks)
    Ball = np.stack([np.random.default_rng(1 + j).standard_normal(rows) for j in range(kmax)])
    runs = []
    for kind in kinds:
        if kind == "multigrid":
            block = B.Precond.multigrid_multi(op, 1, max_rhs=kmax) if dim == 2 else B.Precond.multigrid3d_multi(op, 1, max_rhs=kmax)
            single = B.Precond.multigrid(op, 1) if dim == 2 else B.Precond.multigrid3d(op, 1)
        else:
            block = single = B.Precond(op, kind)
        for k in ks:
            Bk, X0 = Ball[:k], np.zeros((k, rows))
            seen = {}

            def batched():
                X, _, stats = B.gcr_solve_multi(op, mat, block, Bk, X0, restart=16, tol=1e-8, max_iters=20000)
                seen["batched"] = ([s.iterations for s in stats], [int(s.converged) for s in stats], X)
                return stats[0].time_total_ms

            def singles():
                total, its = 0.0, []
                for j in range(k):
                    _, _, st = B.gcr_solve(op, mat, single, Bk[j], X0[j], restart=16, tol=1e-8, max_iters=20000)
                    total += st.time_total_ms
                    its.append(st.iterations)
                seen["single"] = its
                return total

            tb, ts, ratio = alternate(batched, singles)
            its, conv, X = seen["batched"]
            true_rel = [float(np.linalg.norm(Bk[j] - A @ X[j]) / np.linalg.norm(Bk[j])) for j in range(k)]
            rec = {"kind": kind, "k": k, "batched_ms": spread(tb), "singles_ms": spread(ts), "single_over_batched": ratio, "iterations": its,
                   "single_iterations": seen["single"], "converged": conv, "true_relative_residual": true_rel}
            runs.append(rec)
            say(f"upwind {g}^{dim} {op.variant()} GCR(16)+{kind}{'1' if kind == 'multigrid' else ''} k={k}: batched ms median={np.median(tb):.2f} "
                f"range={min(tb):.2f}..{max(tb):.2f}; {k} singles ms median={np.median(ts):.2f} range={min(ts):.2f}..{max(ts):.2f}; single / batched "
                f"{ratio['median']:.3f} (pairwise {ratio['min']:.3f}..{ratio['max']:.3f}); iterations batched {its} single {seen['single']}, "
                f"converged {conv}, true ||b - A x|| / ||b|| <= {max(true_rel):.2e}")
        block.destroy()
        if single is not block:
            single.destroy()
    op.free()
    return {"n": g, "dim": dim, "px": px, "py": py, "pz": pz if dim == 3 else None, "shift": shift, "tol": 1e-8, "restart": 16, "runs": runs}


if upwind_n > 0:
    result["upwind"] = upwind(2, upwind_n)
if cube_n > 0:
    result["cube"] = upwind(3, cube_n)
finish()
