"""Batched preconditioned CG measured (spmv_amd_pcg_solve_device_multi).
   python tools/pcg_multi_bench.py [n=20000] [--ks 1,2,4,8] [--solves 5] [--small 2000] [--skip-small] [--out FILE]
1. The headline grid on stencil5-csr (synthetic +5 / -1, tol 1e-6, right-hand sides b_j = (1 + j/8) * 1 + 0.01 * sin(1e-3 * i),
   x0 = 0): spmv_amd_pcg_solve_device ("jacobi", column 0), batched CG and batched Jacobi-PCG for every k, alternated IN ONE
   PROCESS (hipMalloc's placement decides a few percent per process), 1 warm-up + --solves timed solves each;
   system-iterations per second = the sum of all columns' iterations / time_total_ms, median with min - max. Model, bytes per
   interior row and iteration per system: single "jacobi" 136, batched CG (40 + 80 k) / k, batched "jacobi" (56 + 80 k) / k. Where
   the three workspaces do not fit side by side they are released between the solvers (allocation is outside time_total_ms).
2. --small grid, k = 4, through stencil5-csr: time to solution of batched CG against batched Jacobi-PCG on the scaled stencil
   S A S, s_i = 10^U(0, 2) (seed 1), b_j as above; and batched Chebyshev-PCG of degree 4 on the Poisson stencil (+4 / -1) against
   four single-RHS Chebyshev solves (1 warm-up + 3 timed each, medians).
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
ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]
solves = opt("--solves", 5)
small_n = opt("--small", 2000)
out_path = opt("--out", "")
B.require_gpu()
B.lib().spmv_amd_set_device(0)
result = {"n": n, "solves": solves, "ks": ks}


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def rhs(N, k):
    wiggle = 0.01 * np.sin(1e-3 * np.arange(N, dtype=np.float64))
    return np.stack([(1.0 + j / 8.0) + wiggle for j in range(k)])


# ---- 1. headline grid: system-iterations per second, the three solvers alternated ----
N = n * n
op = B.Operator("stencil5-csr")
assert op.init_synthetic(n) == 0
print(f"grid {n}^2 ({N} rows), operator stencil5-csr, variant {op.variant()}, SpMM kernel {op.spmm_variant()}", flush=True)
m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)  # the solvers read mat->rows only
jac = B.Precond(op, "jacobi")
result["headline"] = {"operator": op.variant(), "spmm": op.spmm_variant(), "by_k": []}
print(f"{'k':>2} {'solver':>14} {'iterations':>26} {'sys-it/s median':>16} {'min':>9} {'max':>9} {'x single':>9} {'model':>7}")
for k in ks:
    Bk = rhs(N, k)
    X0 = np.zeros((k, N))
    tight = (5 + 8 * k + 6) * N * 8 > 150e9  # single PCG, two batched workspaces and the operator side by side

    def run(which):
        if tight:
            B.lib().spmv_amd_cg_release_workspace()
        if which == "single":
            _, _, st = B.pcg_solve_device(op, m, jac, Bk[0], X0[0])
            stats = [st]
        elif which == "cg_multi":
            _, _, stats = B.cg_solve_multi(op, m, Bk, X0)
        else:
            _, _, stats = B.pcg_solve_multi(op, m, jac, Bk, X0)
        assert all(s.converged == 1 for s in stats), which
        its = [s.iterations for s in stats]
        return sum(its) / (stats[0].time_total_ms / 1e3), its

    order = ["single", "cg_multi", "pcg_multi"]
    for w in order:  # warm-up
        run(w)
    rates, iters = {w: [] for w in order}, {}
    for _ in range(solves):
        for w in order:
            rate, iters[w] = run(w)
            rates[w].append(rate)
    rec = {"k": k, "released_between_solvers": bool(tight), "iterations": iters, "rates": rates, "system_iterations_per_s": {w: spread(rates[w]) for w in order}}
    model = {"single": 1.0, "cg_multi": 136.0 / ((40 + 80 * k) / k), "pcg_multi": 136.0 / ((56 + 80 * k) / k)}
    base = rec["system_iterations_per_s"]["single"]["median"]
    for w in order:
        s = rec["system_iterations_per_s"][w]
        print(f"{k:2d} {w:>14} {str(iters[w]):>26} {s['median']:16.2f} {s['min']:9.2f} {s['max']:9.2f} {s['median'] / base:9.3f} {model[w]:7.3f}", flush=True)
    rec["ratio_to_single"] = {w: rec["system_iterations_per_s"][w]["median"] / base for w in order}
    rec["model_ratio_to_single"] = model
    rec["ranges_apart"] = rec["system_iterations_per_s"]["pcg_multi"]["min"] > rec["system_iterations_per_s"]["single"]["max"]
    result["headline"]["by_k"].append(rec)
    del Bk, X0
jac.destroy()
op.free()

# ---- 2. time to solution at k = 4 ----
if "--skip-small" not in sys.argv:
    import scipy.sparse as sp

    g, k = small_n, 4
    G = g * g
    Bk, X0 = rhs(G, k), np.zeros((k, G))

    def stencil(center):
        t = sp.diags([np.full(g - 1, -1.0), np.full(g, center), np.full(g - 1, -1.0)], [-1, 0, 1])
        return sp.kron(sp.identity(g), t) + sp.kron(sp.diags([np.full(g - 1, -1.0), np.full(g - 1, -1.0)], [-1, 1]), sp.identity(g))

    def operator_of(A):
        A = sp.coo_matrix(A)
        order = np.lexsort((A.col, A.row))
        e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
        e["row"], e["col"], e["value"] = A.row[order], A.col[order], A.data[order]
        B.lib().spmv_amd_reset_host_matrices()
        hm = B.HostMatrix(e, G, G, g)
        o = B.Operator("stencil5-csr")
        assert o.init(hm) == 0
        return o, hm

    def timed(fn):
        fn()
        return [fn() for _ in range(3)]

    S = sp.diags(10.0 ** np.random.default_rng(1).uniform(0.0, 2.0, G))
    op, hm = operator_of(S @ stencil(5.0) @ S)
    pc = B.Precond(op, "jacobi")
    tts = {}
    for name, fn in (("cg_multi", lambda: B.cg_solve_multi(op, hm, Bk, X0, max_iters=100000)[2]),
                     ("pcg_multi_jacobi", lambda: B.pcg_solve_multi(op, hm, pc, Bk, X0, max_iters=100000)[2])):
        runs = timed(fn)
        assert all(s.converged == 1 for r in runs for s in r), name
        tts[name] = {"iterations": [s.iterations for s in runs[0]], "ms": float(np.median([r[0].time_total_ms for r in runs]))}
        print(f"scaled {g}^2 d=2 k=4 {op.spmm_variant()} {name:18s} iterations={tts[name]['iterations']} ms={tts[name]['ms']:.2f}", flush=True)
    tts["speedup"] = tts["cg_multi"]["ms"] / tts["pcg_multi_jacobi"]["ms"]
    print(f"time to solution: batched jacobi is {tts['speedup']:.1f}x faster than batched CG")
    result["scaled"] = dict(tts, n=g, decades=2, seed=1, k=k)
    pc.destroy()
    op.free()

    op, hm = operator_of(stencil(4.0))
    pc = B.Precond.chebyshev(op, 4)
    runs = timed(lambda: B.pcg_solve_multi(op, hm, pc, Bk, X0, max_iters=100000)[2])
    assert all(s.converged == 1 for r in runs for s in r)
    batched = {"iterations": [s.iterations for s in runs[0]], "ms": float(np.median([r[0].time_total_ms for r in runs]))}
    singles = timed(lambda: [B.pcg_solve_device(op, hm, pc, Bk[j], X0[j], max_iters=100000)[2] for j in range(k)])
    assert all(s.converged == 1 for r in singles for s in r)
    four = {"iterations": [s.iterations for s in singles[0]], "ms": float(np.median([sum(s.time_total_ms for s in r) for r in singles]))}
    print(f"poisson {g}^2 chebyshev degree 4 k=4: batched iterations={batched['iterations']} ms={batched['ms']:.2f}; four single solves "
          f"iterations={four['iterations']} ms={four['ms']:.2f}; batched is {four['ms'] / batched['ms']:.2f}x", flush=True)
    result["poisson"] = {"n": g, "degree": 4, "k": k, "batched": batched, "four_single": four, "speedup": four["ms"] / batched["ms"]}
    pc.destroy()
    op.free()

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
