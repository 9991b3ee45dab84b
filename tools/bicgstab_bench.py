"""BiCGSTAB measured against PCG (spmv_amd_bicgstab_solve_device). A tool, not a test.
   python tools/bicgstab_bench.py [n=20000] [--solves 5] [--upwind 2000] [--skip-upwind] [--out FILE]
1. The headline grid on stencil5-csr (synthetic +5 / -1: BiCGSTAB runs on a symmetric definite matrix too, and the bytes do not
   depend on the values), b = 1, x0 = 0: BiCGSTAB and spmv_amd_pcg_solve_device, kinds "none" and "jacobi", alternated IN ONE
   PROCESS (hipMalloc's placement decides a few percent per process). Every solve runs a fixed number of
   whole iterations (a tolerance that is never met: 8 of BiCGSTAB, 16 of PCG -- the same number of products, so the initial residual
   weighs the same in both), 1 warm-up + --solves timed solves each; median and range of time_total_ms / iterations.
   Model: 256 B/row against 120 ("none": 2.13 x a PCG iteration), 296 against 136 ("jacobi": 2.18 x).
2. Time to solution on the --upwind grid of the 5-point upwind convection-diffusion stencil (centre 7, W -3, N -1.5, E = S = -1;
   entries built on the host), b = standard_normal(seed 1), x0 = 0, tol 1e-8, both kinds: iterations and ms (1 warm-up + 3 timed
   solves each, median and range), and the true relative residual of the solution in float64.
Prints one line per measurement and a JSON summary; --out FILE gets both."""
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
out_path = opt("--out", "")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


B.require_gpu()
B.lib().spmv_amd_set_device(0)
result = {"n": n, "solves": solves}
MODEL = {"none": 256.0 / 120.0, "jacobi": 296.0 / 136.0}
ITERATIONS = {"bicgstab": 8, "pcg": 16}

# ---- 1. headline grid: ms per iteration, the four loops alternated ----
N = n * n
op = B.Operator("stencil5-csr")
assert op.init_synthetic(n) == 0
m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)
b = np.ones(N)
x0 = np.zeros(N)
pcs = {"none": B.Precond(op, "none"), "jacobi": B.Precond(op, "jacobi")}


def run(solver, kind):
    fn = B.bicgstab_solve if solver == "bicgstab" else B.pcg_solve_device
    _, h, st = fn(op, m, pcs[kind], b, x0, tol=1e-300, max_iters=ITERATIONS[solver])
    assert st.iterations == ITERATIONS[solver] and np.all(np.isfinite(h)), (solver, kind, st.iterations)
    return st.time_total_ms / st.iterations, h[-1] / h[0]


order = [(s, k) for k in ("none", "jacobi") for s in ("pcg", "bicgstab")]
for w in order:  # warm-up
    run(*w)
samples = {w: [] for w in order}
reached = {}
for _ in range(solves):
    for w in order:
        ms, rel = run(*w)
        samples[w].append(ms)
        reached[w] = rel
per_iter = {w: float(np.median(samples[w])) for w in order}
for w in order:
    say(f"{w[0]:8s} {w[1]:6s} iterations={ITERATIONS[w[0]]:2d} ms/iteration median={per_iter[w]:.4f} range={min(samples[w]):.4f}..{max(samples[w]):.4f} "
        f"(||r||/||r0|| reached {reached[w]:.1e})")
ratio = {}
for kind in ("none", "jacobi"):
    r = [bi / pc for bi, pc in zip(samples[("bicgstab", kind)], samples[("pcg", kind)])]
    ratio[kind] = {"median": per_iter[("bicgstab", kind)] / per_iter[("pcg", kind)], "min": min(r), "max": max(r), "model": MODEL[kind]}
    say(f"BiCGSTAB / PCG iteration, kind {kind}: {ratio[kind]['median']:.3f} (pairwise {min(r):.3f}..{max(r):.3f}; model {MODEL[kind]:.2f}, "
        f"measured / model {ratio[kind]['median'] / MODEL[kind]:.3f})")
result["headline"] = {"operator": op.variant(), "iterations": ITERATIONS, "ms_per_iteration": {f"{s}+{k}": v for (s, k), v in per_iter.items()},
                      "samples": {f"{s}+{k}": v for (s, k), v in samples.items()}, "ratio": ratio}
for p in pcs.values():
    p.destroy()
op.free()

# ---- 2. time to solution on the upwind stencil ----
if "--skip-upwind" not in sys.argv:
    import scipy.sparse as sp

    k = upwind_n
    px, py, shift = 2.0, 0.5, 0.5
    t = sp.diags([np.full(k - 1, -1.0 - px), np.full(k, 4.0 + px + py + shift), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = sp.csr_matrix(sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0 - py), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k)))
    c = sp.coo_matrix(A)
    pick = np.lexsort((c.col, c.row))
    e = np.zeros(c.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = c.row[pick], c.col[pick], c.data[pick]
    B.lib().spmv_amd_reset_host_matrices()
    mu = B.HostMatrix(e, k * k, k * k, k)
    op = B.Operator("stencil5-csr")
    assert op.init(mu) == 0
    bb, xx = np.random.default_rng(1).standard_normal(k * k), np.zeros(k * k)
    tts = {}
    for kind in ("none", "jacobi"):
        pc = B.Precond(op, kind)
        B.bicgstab_solve(op, mu, pc, bb, xx, tol=1e-8, max_iters=10000)
        runs = [B.bicgstab_solve(op, mu, pc, bb, xx, tol=1e-8, max_iters=10000) for _ in range(3)]
        assert all(r[2].converged == 1 for r in runs), kind
        ms = [r[2].time_total_ms for r in runs]
        true_rel = float(np.linalg.norm(bb - A @ runs[0][0]) / np.linalg.norm(bb))
        tts[kind] = {"iterations": runs[0][2].iterations, "ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "true_relative_residual": true_rel}
        say(f"upwind {k}^2 {op.variant()} bicgstab+{kind:6s} iterations={tts[kind]['iterations']:4d} ms median={tts[kind]['ms']:.2f} "
            f"range={min(ms):.2f}..{max(ms):.2f} true ||b - A x|| / ||b|| = {true_rel:.2e}")
        pc.destroy()
    result["upwind"] = dict(tts, n=k, px=px, py=py, shift=shift, tol=1e-8, operator=op.variant())
    op.free()

say(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
