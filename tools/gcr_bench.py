"""GCR(m) measured against BiCGSTAB (spmv_amd_gcr_solve_device). A tool, not a test.
   python tools/gcr_bench.py [n=20000] [--solves 5] [--upwind 2000] [--cube 0] [--skip-headline] [--skip-upwind] [--out FILE]
   python tools/gcr_bench.py [n=20000] --stages 15 [--calls 5]
1. The headline grid on stencil5-csr (synthetic +5 / -1: the bytes do not depend on the values), b = 1, x0 = 0: GCR at restart 4
   and 16 and BiCGSTAB, kinds "none" and "jacobi", alternated IN ONE PROCESS (hipMalloc's placement decides a few percent per
   process). Every solve runs a fixed number of whole iterations under a tolerance that is never met: 16 of GCR
   (four restart cycles of 4, one of 16) and 8 of BiCGSTAB -- 16 products each, so the initial residual weighs the same --, 1 warm-up
   + --solves timed solves each; median and range of time_total_ms per PRODUCT. Model, bytes per row and product: BiCGSTAB 128
   ("jacobi" 148); GCR slot 0 128 (152), slot j 144 + 24 j (168 + 24 j): 176 (200) as the mean of a cycle of 4, 323 (347) of 16.
2. Time to solution on the --upwind grid of the 5-point upwind convection-diffusion stencil with px = 2, py = 0.5, shift = 0 (centre
   6.5, W -3, N -1.5, E = S = -1; entries built on the host), b = standard_normal(seed 1), x0 = 0, tol 1e-8: GCR(16) + multigrid
   (nu = 1), GCR(16) + jacobi and BiCGSTAB + jacobi; iterations and ms (1 warm-up + 3 timed solves each, median and range), and the
   true relative residual of the solution in float64. --cube N: the same on the N^3 7-point twin (pz = 1) on stencil7-csr.
--stages J: nothing of the above; --calls launches each of the multidot and orthogonalise kernels at slot J and of the x / r kernel
   through the LAB build's spmv_amd_gcr_stage on the headline grid, for a profiler's per-kernel times (bytes per row: multidot
   8 (J + 1), orthogonalise 32 + 16 J, x / r 48).
Prints one line per measurement and a JSON summary; --out FILE gets both."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
n = int(args[0]) if args else 20000
solves = opt("--solves", 5)
upwind_n = opt("--upwind", 2000)
cube_n = opt("--cube", 0)
stage_slot = opt("--stages", -1)
calls = opt("--calls", 5)
out_path = opt("--out", "")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


N = n * n

if stage_slot >= 0:
    # ---- the three streaming kernels alone, for a profiler ----
    L = B.use_lab()
    L.require_gpu()
    L.lib().spmv_amd_set_device(0)
    j = stage_slot
    assert 1 <= j < L.GCR_MAX_RESTART
    vectors = [L.DeviceVector(N, 1.0 / (i + 1)) for i in range(2 * (j + 1) + 2)]
    Q = (C.c_void_p * L.GCR_MAX_RESTART)(*([v.ptr for v in vectors[:j + 1]] + [None] * (L.GCR_MAX_RESTART - j - 1)))
    Z = (C.c_void_p * L.GCR_MAX_RESTART)(*([v.ptr for v in vectors[j + 1:2 * (j + 1)]] + [None] * (L.GCR_MAX_RESTART - j - 1)))
    x, r = vectors[-2], vectors[-1]
    count = max(1, ((N >> 1) + 63) // 64)
    partials = L.DeviceVector(L.GCR_MAX_RESTART * count, 0.0)
    a = L.GcrStageArgs(n=N, x=x.ptr, r=r.ptr, z_in=r.ptr, Q=Q, Z=Z, slot=j, partials=partials.ptr)
    sc = L.GcrScalars()
    sc.alpha = 1e-3
    for i in range(j):
        sc.beta[i] = 1e-3
    for _ in range(calls):
        for stage in ("multidot", "orthogonalise", "update_xr"):
            assert L.gcr_stage(stage, "none", a, sc) == 0
    say(f"stages at slot {j} on {n}^2 rows: {calls} launches each of gcr_multidot_kernel ({8 * (j + 1)} B/row), "
        f"gcr_orthogonalise_kernel ({32 + 16 * j} B/row) and gcr_update_xr_kernel (48 B/row)")
    for v in vectors + [partials]:
        v.free()
    sys.exit(0)

B.require_gpu()
B.lib().spmv_amd_set_device(0)
result = {"n": n, "solves": solves}
PRODUCTS = 16
BYTES = {("bicgstab", "none"): 128.0, ("bicgstab", "jacobi"): 148.0, ("gcr4", "none"): 176.0, ("gcr4", "jacobi"): 200.0,
         ("gcr16", "none"): 323.0, ("gcr16", "jacobi"): 347.0}

# ---- 1. headline grid: ms per product, the six loops alternated ----
if "--skip-headline" not in sys.argv:
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)
    b = np.ones(N)
    x0 = np.zeros(N)
    pcs = {"none": B.Precond(op, "none"), "jacobi": B.Precond(op, "jacobi")}

    def run(solver, kind):
        if solver == "bicgstab":
            _, h, st = B.bicgstab_solve(op, m, pcs[kind], b, x0, tol=1e-300, max_iters=PRODUCTS // 2)
            products = 2 * st.iterations
        else:
            _, h, st = B.gcr_solve(op, m, pcs[kind], b, x0, restart=int(solver[3:]), tol=1e-300, max_iters=PRODUCTS)
            products = st.iterations
        assert products == PRODUCTS and np.all(np.isfinite(h)), (solver, kind, st.iterations)
        return st.time_total_ms / products, h[-1] / h[0]

    order = [(s, k) for k in ("none", "jacobi") for s in ("bicgstab", "gcr4", "gcr16")]
    for w in order:  # warm-up
        run(*w)
    samples = {w: [] for w in order}
    reached = {}
    for _ in range(solves):
        for w in order:
            ms, rel = run(*w)
            samples[w].append(ms)
            reached[w] = rel
    per = {w: float(np.median(samples[w])) for w in order}
    for w in order:
        say(f"{w[0]:8s} {w[1]:6s} products={PRODUCTS} ms/product median={per[w]:.4f} range={min(samples[w]):.4f}..{max(samples[w]):.4f} "
            f"model {BYTES[w]:.0f} B/row = {BYTES[w] * N / per[w] / 1e6:.0f} GB/s (||r||/||r0|| reached {reached[w]:.1e})")
    ratio = {}
    for kind in ("none", "jacobi"):
        for s in ("gcr4", "gcr16"):
            pair = [g / bi for g, bi in zip(samples[(s, kind)], samples[("bicgstab", kind)])]
            model = BYTES[(s, kind)] / BYTES[("bicgstab", kind)]
            ratio[f"{s}+{kind}"] = {"median": per[(s, kind)] / per[("bicgstab", kind)], "min": min(pair), "max": max(pair), "model": model}
            say(f"{s} / BiCGSTAB per product, kind {kind}: {ratio[f'{s}+{kind}']['median']:.3f} (pairwise {min(pair):.3f}..{max(pair):.3f}; "
                f"model {model:.3f}, measured / model {ratio[f'{s}+{kind}']['median'] / model:.3f})")
    result["headline"] = {"operator": op.variant(), "products": PRODUCTS, "ms_per_product": {f"{s}+{k}": v for (s, k), v in per.items()},
                          "samples": {f"{s}+{k}": v for (s, k), v in samples.items()}, "ratio": ratio}
    for p in pcs.values():
        p.destroy()
    op.free()


# ---- 2. time to solution on the upwind stencils ----
def upwind(dim, k):
    import scipy.sparse as sp

    px, py, pz, shift = 2.0, 0.5, 1.0, 0.0
    eye = sp.identity(k)
    lower = lambda p: sp.diags([np.full(k - 1, -1.0 - p), np.full(k - 1, -1.0)], [-1, 1])
    if dim == 2:
        t = sp.diags([np.full(k - 1, -1.0 - px), np.full(k, 4.0 + px + py + shift), np.full(k - 1, -1.0)], [-1, 0, 1])
        A = sp.csr_matrix(sp.kron(eye, t) + sp.kron(lower(py), eye))
    else:
        t = sp.diags([np.full(k - 1, -1.0 - px), np.full(k, 6.0 + px + py + pz + shift), np.full(k - 1, -1.0)], [-1, 0, 1])
        A = sp.csr_matrix(sp.kron(eye, sp.kron(eye, t)) + sp.kron(eye, sp.kron(lower(py), eye)) + sp.kron(lower(pz), sp.kron(eye, eye)))
    rows = A.shape[0]
    c = sp.coo_matrix(A)
    pick = np.lexsort((c.col, c.row))
    e = np.zeros(c.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = c.row[pick], c.col[pick], c.data[pick]
    B.lib().spmv_amd_reset_host_matrices()
    mu = B.HostMatrix(e, rows, rows, k)
    op = B.Operator("stencil5-csr" if dim == 2 else "stencil7-csr")
    assert op.init(mu) == 0
    bb, xx = np.random.default_rng(1).standard_normal(rows), np.zeros(rows)
    contestants = (("gcr16+multigrid1", lambda: B.Precond.multigrid(op, 1) if dim == 2 else B.Precond.multigrid3d(op, 1), True),
                   ("gcr16+jacobi", lambda: B.Precond(op, "jacobi"), True), ("bicgstab+jacobi", lambda: B.Precond(op, "jacobi"), False))
    tts = {}
    for name, make, is_gcr in contestants:
        pc = make()
        solve = (lambda: B.gcr_solve(op, mu, pc, bb, xx, restart=16, tol=1e-8, max_iters=20000)) if is_gcr else \
            (lambda: B.bicgstab_solve(op, mu, pc, bb, xx, tol=1e-8, max_iters=20000))
        solve()
        runs = [solve() for _ in range(3)]
        ms = [r[2].time_total_ms for r in runs]
        true_rel = float(np.linalg.norm(bb - A @ runs[0][0]) / np.linalg.norm(bb))
        tts[name] = {"iterations": runs[0][2].iterations, "converged": int(runs[0][2].converged), "ms": float(np.median(ms)), "ms_min": min(ms),
                     "ms_max": max(ms), "true_relative_residual": true_rel}
        say(f"upwind {k}^{dim} {op.variant()} {name:17s} iterations={tts[name]['iterations']:5d} converged={tts[name]['converged']} "
            f"ms median={tts[name]['ms']:.2f} range={min(ms):.2f}..{max(ms):.2f} true ||b - A x|| / ||b|| = {true_rel:.2e}")
        pc.destroy()
    op.free()
    return dict(tts, n=k, px=px, py=py, pz=pz if dim == 3 else None, shift=shift, tol=1e-8)


if "--skip-upwind" not in sys.argv:
    result["upwind"] = upwind(2, upwind_n)
if cube_n > 0:
    result["cube"] = upwind(3, cube_n)

say(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
