"""Several right-hand sides per matrix pass, measured: the STENCIL5 SpMM (spmv_amd_spmm_device) and the batched CG
(spmv_amd_cg_solve_device_multi) for k = 1, 2, 4, 8 on one operator, beside the single-vector SpMV and cg_solve_device on one
column IN THE SAME PROCESS (hipMalloc's placement decides a few percent per process, DESIGN.md section 2: numbers from two
processes are not compared).
   python tools/multi_rhs_bench.py [n=20000] [--ks 1,2,4,8]
SpMM: 5 warm-up + 10 launches timed one by one with HIP events on the default stream, >2 sigma dropped, median (the reference
rule); reported as algorithmic GB/s at (40 + 16 k) B per interior row and as a fraction of 8 TB/s.
CG: right-hand sides b_j = (1 + j/8) * 1 + 0.01 * sin(1e-3 * i) (i = row, j = column), x0 = 0; 1 warm-up + 3 timed solves,
median of time_total_ms (the whole batch); system-iterations/s = the sum of all columns' iterations / wall time.
Model, bytes per interior row and iteration per system: SpMM (40 + 16 k) / k, CG (40 + 80 k) / k."""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 20000
ks = [1, 2, 4, 8]
if "--ks" in sys.argv:
    ks = [int(v) for v in sys.argv[sys.argv.index("--ks") + 1].split(",")]
N = n * n
interior = (n - 2) * (n - 2)
PEAK = 8.0e12
B.require_gpu()
L = B._multi_lib()


def rule(ms):
    t = np.asarray(ms, dtype=np.float64)
    keep = t[np.abs(t - t.mean()) <= 2.0 * t.std()] if t.std() > 0 else t
    return float(np.median(keep))


# HIP events on the default stream, through the runtime the library already loaded
_hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))


def event_ms(launch, warmup=5, reps=10):
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert _hip.hipEventCreate(C.byref(e0)) == 0 and _hip.hipEventCreate(C.byref(e1)) == 0
    for _ in range(warmup):
        launch()
    out = []
    for _ in range(reps):
        _hip.hipEventRecord(e0, None)
        launch()
        _hip.hipEventRecord(e1, None)
        assert _hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        _hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        out.append(ms.value)
    _hip.hipEventDestroy(e0), _hip.hipEventDestroy(e1)
    return rule(out)


op = B.Operator("stencil5-csr")
assert op.init_synthetic(n) == 0
print(f"grid {n}^2 ({N} rows), operator stencil5-csr, variant {op.variant()}, SpMM kernel {op.spmm_variant()}", flush=True)
result = {"grid": n, "rows": N, "variant": op.variant(), "spmm_variant": op.spmm_variant(), "spmm": [], "cg": []}

# ---- SpMV / SpMM ----
dx1, dy1 = B.DeviceVector(N, fill=1.0), B.DeviceVector(N, fill=0.0)
spmv_ms = event_ms(lambda: op.run_device(dx1, dy1))
dx1.free(), dy1.free()
gbs1 = (40 + 16) * interior / spmv_ms / 1e6
print(f"single SpMV (run_device): {spmv_ms:.3f} ms  {gbs1:7.1f} GB/s  {gbs1 * 1e9 / PEAK:.3f} of 8 TB/s", flush=True)
result["spmv_ms"] = spmv_ms
print(f"{'k':>2} {'SpMM ms':>9} {'x SpMV':>7} {'model x':>8} {'GB/s':>8} {'of 8TB/s':>9} {'ms/system':>10}")
for k in ks:
    X, Y = B.DeviceBlock(k, N), B.DeviceBlock(k, N)
    L.spmv_amd_device_fill_f64(X.ptr, N * k, 1.0)
    ms = event_ms(lambda: L.spmv_amd_spmm_device(b"stencil5-csr", k, X.ptr, Y.ptr))
    X.free(), Y.free()
    gbs = (40 + 16 * k) * interior / ms / 1e6
    rec = {"k": k, "ms": ms, "ratio_to_spmv": ms / spmv_ms, "model_ratio": (40 + 16 * k) / 56.0, "gb_s": gbs, "fraction_of_8tbs": gbs * 1e9 / PEAK,
           "ms_per_system": ms / k}
    result["spmm"].append(rec)
    print(f"{k:2d} {ms:9.3f} {rec['ratio_to_spmv']:7.3f} {rec['model_ratio']:8.3f} {gbs:8.1f} {rec['fraction_of_8tbs']:9.3f} {ms / k:10.3f}", flush=True)

# ---- CG ----
shell = B.HostMatrix(np.empty(0, dtype=B.ENTRY_DTYPE), N, N, n)  # the solvers read mat->rows only
wiggle = 0.01 * np.sin(1e-3 * np.arange(N, dtype=np.float64))


def rhs(j):
    return (1.0 + j / 8.0) + wiggle


b0 = rhs(0)
runs = []
for i in range(4):
    x, hist, st = B.cg_solve(op, shell, b0, np.zeros(N), device=True)
    if i:
        runs.append(st.time_total_ms)
single_ms = rule(runs)
single_rate = st.iterations / (single_ms / 1e3)
result["cg_single"] = {"ms": single_ms, "iterations": st.iterations, "system_iterations_per_s": single_rate}
print(f"cg_solve_device, column 0: {single_ms:.3f} ms, {st.iterations} iterations, {single_rate:.2f} system-iterations/s", flush=True)
del x
B.lib().spmv_amd_cg_release_workspace()  # room for the batched workspaces

# model of the gain per system: today's single-RHS loop moves 40 + 72 = 112 B per interior row and iteration (SpMM, r update 24,
# direction update 24, deferred x update 8); this loop moves (40 + 80 k) / k (x folded into the direction update, no ring), which
# is 120 B at k = 1. Both bases are printed.
print(f"{'k':>2} {'wall ms':>9} {'iterations':>24} {'sys-it/s':>9} {'x single':>9} {'model/112B':>10} {'model/120B':>10}")
for k in ks:
    Bk = np.empty((k, N))
    for j in range(k):
        Bk[j] = rhs(j)
    runs = []
    for i in range(4):
        X, hists, stats = B.cg_solve_multi(op, shell, Bk, np.zeros((k, N)))
        if i:
            runs.append(stats[0].time_total_ms)
        del X
    ms = rule(runs)
    its = [s.iterations for s in stats]
    rate = sum(its) / (ms / 1e3)
    per_system = (40 + 80 * k) / k
    rec = {"k": k, "ms": ms, "iterations": its, "converged": [s.converged for s in stats], "system_iterations_per_s": rate,
           "ratio_to_single": rate / single_rate, "model_ratio_vs_112B": 112 / per_system, "model_ratio_vs_120B": 120 / per_system}
    result["cg"].append(rec)
    print(f"{k:2d} {ms:9.3f} {str(its):>24} {rate:9.2f} {rate / single_rate:9.3f} {112 / per_system:10.3f} {120 / per_system:10.3f}",
          flush=True)
    del Bk
op.free()
print(json.dumps(result))
