"""Batched BiCGSTAB measured against k single-RHS solves (spmv_amd_bicgstab_solve_device_multi). A tool, not a test.
   python tools/bicgstab_multi_bench.py [n=2000] [--ks 1,2,4,8] [--iterations 8] [--solves 5] [--out FILE] [--trace DIR]
The system of tools/bicgstab_bench.py's headline (stencil5-csr, synthetic +5 / -1: the bytes do not depend on the values), right-hand
sides b_j = (1 + j/8) + 0.01 * sin(1e-3 * i), x0 = 0. For each kind ("none", "jacobi") and each k: ONE batched solve against k
spmv_amd_bicgstab_solve_device solves, alternated IN ONE PROCESS (hipMalloc's placement decides a few percent per process, DESIGN.md
section 2), every solve a fixed number of whole iterations (a tolerance that is never met), 1 warm-up + --solves timed rounds;
time_total_ms of the batch against the sum of the k singles' (upload and download are outside both). Reported: ms per system and
iteration, median and range, and the ratio single / batched with its pairwise range beside the byte model per row, column and
iteration: "none" 256 against 144 + 2 (40 / k + 16); "jacobi" 296 against 168 + 16 / k + 2 (40 / k + 16).
--trace DIR: one more run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process: k = the last of --ks, kind
"jacobi", one round) writing under DIR, and the per-kernel rows of its statistics.
Prints one line per measurement and a JSON summary; --out FILE gets both."""
import csv
import glob
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
n = int(args[0]) if args else 2000
ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]
iterations = opt("--iterations", 8)
solves = opt("--solves", 5)
out_path = opt("--out", "")
trace_dir = opt("--trace", "")
kinds = opt("--kinds", "none,jacobi").split(",")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def model(kind, k):
    """Bytes per row, column and iteration: the single solver's over the batched solver's."""
    if kind == "none":
        return 256.0 / (144.0 + 2.0 * (40.0 / k + 16.0))
    return 296.0 / (168.0 + 16.0 / k + 2.0 * (40.0 / k + 16.0))


def rhs(N, k):
    wiggle = 0.01 * np.sin(1e-3 * np.arange(N, dtype=np.float64))
    return np.stack([(1.0 + j / 8.0) + wiggle for j in range(k)])


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


B.require_gpu()
B.lib().spmv_amd_set_device(0)
N = n * n
op = B.Operator("stencil5-csr")
assert op.init_synthetic(n) == 0
m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)  # the solvers read mat->rows only
say(f"grid {n}^2 ({N} rows), operator stencil5-csr, variant {op.variant()}, SpMM kernel {op.spmm_variant()}, {iterations} iterations per solve")
result = {"n": n, "iterations": iterations, "solves": solves, "operator": op.variant(), "spmm": op.spmm_variant(), "runs": []}
pcs = {kind: B.Precond(op, kind) for kind in kinds}

for kind in kinds:
    for k in ks:
        Bk, X0 = rhs(N, k), np.zeros((k, N))

        def batched():
            _, hists, stats = B.bicgstab_solve_multi(op, m, pcs[kind], Bk, X0, tol=1e-300, max_iters=iterations)
            assert all(s.iterations == iterations for s in stats) and all(np.all(np.isfinite(h)) for h in hists), (kind, k)
            return stats[0].time_total_ms / (iterations * k)

        def singles():
            total = 0.0
            for j in range(k):
                _, h, st = B.bicgstab_solve(op, m, pcs[kind], Bk[j], X0[j], tol=1e-300, max_iters=iterations)
                assert st.iterations == iterations and np.all(np.isfinite(h)), (kind, k, j)
                total += st.time_total_ms
            return total / (iterations * k)

        batched(), singles()  # warm-up
        tb, ts = [], []
        for _ in range(solves):
            tb.append(batched())
            ts.append(singles())
        pair = [s / b for s, b in zip(ts, tb)]
        ratio = float(np.median(ts) / np.median(tb))
        rec = {"kind": kind, "k": k, "batched_ms_per_system_iteration": spread(tb), "single_ms_per_system_iteration": spread(ts),
               "single_over_batched": {"median": ratio, "min": min(pair), "max": max(pair)}, "model": model(kind, k)}
        rec["verdict"] = "met" if ratio >= rec["model"] else "missed"
        result["runs"].append(rec)
        say(f"{kind:6s} k={k}: ms per system and iteration batched {np.median(tb):.4f} ({min(tb):.4f}..{max(tb):.4f}) single {np.median(ts):.4f} "
            f"({min(ts):.4f}..{max(ts):.4f}); single / batched {ratio:.3f} (pairwise {min(pair):.3f}..{max(pair):.3f}; model {rec['model']:.2f}: "
            f"{rec['verdict']}, measured / model {ratio / rec['model']:.3f})")
        del Bk, X0
for p in pcs.values():
    p.destroy()
op.free()

if trace_dir:
    os.makedirs(trace_dir, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), str(n), "--ks", str(ks[-1]), "--kinds", "jacobi", "--iterations", str(iterations), "--solves", "1"]
    done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + child,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    stats = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if done.returncode != 0 or not stats:
        say(f"trace: rocprofv3 exit {done.returncode}, statistics files found: {len(stats)}\n{done.stdout[-2000:]}")
    else:
        rows = list(csv.DictReader(open(stats[-1])))
        result["trace"] = {"k": ks[-1], "kind": "jacobi", "file": os.path.relpath(stats[-1], trace_dir), "kernels": rows[:14]}
        say(f"trace (k = {ks[-1]}, jacobi, warm-up + 1 round, the k single solves included): {stats[-1]}")
        for r in rows[:14]:
            say(f"  {r.get('Name', '?')[:90]:90s} calls={r.get('Calls', '?'):>5s} total_ns={r.get('TotalDurationNs', '?'):>12s} "
                f"avg_ns={r.get('AverageNs', '?'):>12s} {r.get('Percentage', '?'):>6s} %")

say(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
