"""Preconditioned CG measured (spmv_amd_pcg_solve_device).
   python tools/pcg_bench.py [n=20000] [--solves 5] [--scaled 2000] [--skip-scaled] [--out FILE]
1. The headline grid on stencil5-csr (synthetic +5 / -1, b = 1, x0 = 0, tol 1e-6): cg_solve_device, PCG "none" and PCG "jacobi"
   alternated IN ONE PROCESS (hipMalloc's placement decides a few percent per process), 1 warm-up + --solves
   timed solves each; medians of time_total_ms / iterations. Model: 136 B/row ("jacobi"), 120 ("none") against ~113 for
   cg_solve_device, i.e. 1.20x / 1.06x its iteration time.
2. Time to solution on the scaled stencil S A S, s_i = 10^U(0, 2) (seed 1), --scaled grid through cusparse-csr: cg_solve_device
   against "jacobi" PCG, iterations and ms (1 warm-up + 3 timed solves each, medians).
Prints one line per measurement and a JSON summary (also written to --out)."""
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
scaled_n = opt("--scaled", 2000)
out_path = opt("--out", "")
B.require_gpu()
B.lib().spmv_amd_set_device(0)
result = {"n": n, "solves": solves}

# ---- 1. headline grid: ms per iteration, the three loops alternated ----
N = n * n
op = B.Operator("stencil5-csr")
assert op.init_synthetic(n) == 0
m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)
b = np.ones(N)
x0 = np.zeros(N)
pcs = {"none": B.Precond(op, "none"), "jacobi": B.Precond(op, "jacobi")}


def run(which):
    if which == "cg_solve_device":
        _, h, st = B.cg_solve(op, m, b, x0)
    else:
        _, h, st = B.pcg_solve_device(op, m, pcs[which], b, x0)
    assert st.converged == 1, which
    return st.time_total_ms, st.iterations, h


order = ["cg_solve_device", "none", "jacobi"]
for w in order:  # warm-up
    run(w)
samples = {w: [] for w in order}
iters = {}
for _ in range(solves):
    for w in order:
        ms, it, _ = run(w)
        samples[w].append(ms / it)
        iters[w] = it
per_iter = {w: float(np.median(samples[w])) for w in order}
for w in order:
    print(f"{w:16s} iterations={iters[w]:3d} ms/iteration median={per_iter[w]:.4f} all={[round(v, 4) for v in samples[w]]}")
ratio = {w: per_iter[w] / per_iter["cg_solve_device"] for w in ("none", "jacobi")}
print(f"ratio to cg_solve_device: none {ratio['none']:.3f} (model 1.06), jacobi {ratio['jacobi']:.3f} (model 1.20, target <= 1.25)")
result["headline"] = {"operator": op.variant(), "iterations": iters, "ms_per_iteration": per_iter, "samples": samples, "ratio": ratio}
for p in pcs.values():
    p.destroy()
op.free()

# ---- 2. time to solution on the scaled stencil ----
if "--skip-scaled" not in sys.argv:
    import scipy.sparse as sp

    k = scaled_n
    t = sp.diags([np.full(k - 1, -1.0), np.full(k, 5.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k))
    S = sp.diags(10.0 ** np.random.default_rng(1).uniform(0.0, 2.0, k * k))
    A = sp.coo_matrix(S @ A @ S)
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row, A.col, A.data
    B.lib().spmv_amd_reset_host_matrices()
    ms_ = B.HostMatrix(e, k * k, k * k, k)
    op = B.Operator("cusparse-csr")
    assert op.init(ms_) == 0
    pc = B.Precond(op, "jacobi")
    bb, xx = np.ones(k * k), np.zeros(k * k)
    tts = {}
    for name, fn in (("cg_solve_device", lambda: B.cg_solve(op, ms_, bb, xx, max_iters=100000)),
                     ("jacobi", lambda: B.pcg_solve_device(op, ms_, pc, bb, xx, max_iters=100000))):
        fn()
        runs = [fn()[2] for _ in range(3)]
        assert all(s.converged == 1 for s in runs), name
        tts[name] = {"iterations": runs[0].iterations, "ms": float(np.median([s.time_total_ms for s in runs]))}
        print(f"scaled {k}^2 d=2 cusparse-csr {name:16s} iterations={tts[name]['iterations']:6d} ms={tts[name]['ms']:.2f}")
    tts["speedup"] = tts["cg_solve_device"]["ms"] / tts["jacobi"]["ms"]
    print(f"time to solution: jacobi is {tts['speedup']:.1f}x faster")
    result["scaled"] = dict(tts, n=k, decades=2, seed=1, operator=op.variant())
    pc.destroy()
    op.free()

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
