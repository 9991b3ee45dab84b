"""Batched multigrid-preconditioned CG on the 3-D operator measured (spmv_amd_precond_create_multigrid3d_multi).
   python tools/mg3d_multi_bench.py [--grid 256] [--ks 1,2,4,8] [--solves 5] [--out FILE]
   python tools/mg3d_multi_bench.py --cycle-trace [n=512] [--k 4] [--check]      (to be run under a kernel trace)
   python tools/mg3d_multi_bench.py --products [--grids 64,96,128,256,512] [--k 4] [--out FILE]      (LAB build)
1. Time to solution on the Poisson stencil (centre 6, neighbours -1, spmv_amd_init_stencil7_synthetic_values), nu = 1, tol 1e-6, k
   right-hand sides b_j ~ N(0, 1) from x0_j ~ N(0, 1) (seed = the grid): ONE batched solve (spmv_amd_pcg_solve_device_multi on a handle
   of spmv_amd_precond_create_multigrid3d_multi) against k single-RHS solves (spmv_amd_pcg_solve_device on a handle of
   spmv_amd_precond_create_multigrid3d: the existing code, the baseline), alternated IN ONE PROCESS, 1 warm-up + --solves timed rounds;
   medians of time_total_ms (the baseline: the sum over its k solves) with min - max.
2. The wall time of one application (nu = 1, median of 9): spmv_amd_precond_apply_device_multi on k columns against k calls of
   spmv_amd_precond_apply_device. Both synchronise.
3. --cycle-trace: on the same matrix, 3 single-vector V(1, 1) cycles and 3 cycles on --k columns. Run it under
   `rocprofv3 --kernel-trace --stats -- python tools/mg3d_multi_bench.py --cycle-trace` in a run of its own (no counters): the level-0
   launches of residual_restrict3d_multi_kernel<k>, prolong_correct3d_multi_kernel<k> and the block product (the largest duration of
   each name) are to be put beside k launches of residual_restrict3d_kernel, prolong_correct3d_kernel and stencil7_rowlds_kernel.
   --check compares every column of the block result with the single-vector result bit for bit.
4. --products: a level's block product in its two kinds, "spmm/stencil7-row-lds" against "spmm/csr", at --k columns on each grid: two
   one-level hierarchies (max_levels = 1: the application is term 0 and eight smoothing steps, each ONE block product and one step
   kernel) made with the LAB build's spmv_amd_mg3d_multi_level_product forcing one kind each; 2 warm-up + 9 alternated block
   applications, wall time. Everything but the eight products is the same launch sequence, so the difference of the medians / 8 is the
   difference of one product, and a kind is called faster where the two ranges lie apart.
Prints one line per measurement and a JSON summary (also written to --out)."""
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


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def poisson(Bx, n):
    op = Bx.Operator("stencil7-csr")
    assert op.init_synthetic3d(n, 6.0, -1.0) == 0
    return op, Bx.HostMatrix(np.zeros(0, dtype=Bx.ENTRY_DTYPE), n ** 3, n ** 3, n)


out_path = opt("--out", "")

if "--products" in sys.argv:
    L = B.use_lab()
    L.require_gpu()
    L.lib().spmv_amd_set_device(0)
    k = opt("--k", 4)
    result = {"k": k, "products_per_application": 8, "products": []}
    print(f"{'grid':>5} {'stencil7 ms':>12} {'min':>8} {'max':>8} {'csr ms':>10} {'min':>8} {'max':>8} {'per product, csr - stencil7 ms':>31}  stencil7 faster, ranges apart")
    for n in [int(v) for v in opt("--grids", "64,96,128,256,512").split(",")]:
        N = n ** 3
        op, m = poisson(L, n)
        handles = {}
        for kind in ("stencil7", "csr"):
            assert L.mg3d_multi_level_product(kind) == 0
            handles[kind] = L.Precond.multigrid3d_multi(op, 1, 1, k)
            assert handles[kind].multigrid_level_spmm(0) == ("spmm/csr" if kind == "csr" else "spmm/stencil7-row-lds")
        assert L.mg3d_multi_level_product("auto") == 0
        R, Z = L.DeviceVector(N * k, fill=1.0), L.DeviceVector(N * k, fill=0.0)
        times = {"stencil7": [], "csr": []}
        for round_ in range(11):
            for kind, pc in handles.items():
                t0 = time.perf_counter()
                pc.apply_device_multi(op, k, R.ptr, Z.ptr)
                if round_ >= 2:
                    times[kind].append((time.perf_counter() - t0) * 1e3)
        s7, cs = spread(times["stencil7"]), spread(times["csr"])
        rec = {"grid": n, "stencil7_ms": s7, "csr_ms": cs, "per_product_difference_ms": (cs["median"] - s7["median"]) / 8,
               "stencil7_faster_ranges_apart": cs["min"] > s7["max"], "csr_faster_ranges_apart": s7["min"] > cs["max"]}
        result["products"].append(rec)
        print(f"{n:5d} {s7['median']:12.3f} {s7['min']:8.3f} {s7['max']:8.3f} {cs['median']:10.3f} {cs['min']:8.3f} {cs['max']:8.3f} "
              f"{rec['per_product_difference_ms']:31.4f}  {rec['stencil7_faster_ranges_apart']}", flush=True)
        for pc in handles.values():
            pc.destroy()
        R.free(), Z.free()
        op.free()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    sys.exit(0)

B.require_gpu()
B.lib().spmv_amd_set_device(0)

if "--cycle-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--cycle-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 512
    k = opt("--k", 4)
    N = n ** 3
    op, m = poisson(B, n)
    old = B.Precond.multigrid3d(op, 1)
    new = B.Precond.multigrid3d_multi(op, 1, 0, k)
    r, z = B.DeviceVector(N, fill=1.0), B.DeviceVector(N, fill=0.0)
    R, Z = B.DeviceVector(N * k, fill=1.0), B.DeviceVector(N * k, fill=0.0)
    for _ in range(3):
        old.apply_device(op, r.ptr, z.ptr)
    for _ in range(3):
        new.apply_device_multi(op, k, R.ptr, Z.ptr)
    print(f"cycle-trace {n}^3 on {op.variant()}: 3 single V(1,1) cycles, 3 cycles on {k} columns, grids {new.multigrid_info()[1]}")
    if "--check" in sys.argv:
        single = z.to_host()
        block = Z.to_host().reshape(N, k)
        same = all(np.array_equal(single.view(np.uint64), np.ascontiguousarray(block[:, j]).view(np.uint64)) for j in range(k))
        print(f"every column of the block result equals the single-vector result bit for bit: {same}")
        assert same
    old.destroy(), new.destroy()
    for v in (r, z, R, Z):
        v.free()
    op.free()
    sys.exit(0)

solves = opt("--solves", 5)
g = opt("--grid", 256)
ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]
result = {"solves": solves, "n": g, "nu": 1, "tol": 1e-6, "by_k": []}
G = g ** 3
op, m = poisson(B, g)
kmax = max(ks)
rng = np.random.default_rng(g)
Bk = np.empty((kmax, G))
X0 = np.empty((kmax, G))
for j in range(kmax):
    Bk[j], X0[j] = rng.standard_normal(G), rng.standard_normal(G)
old = B.Precond.multigrid3d(op, 1)
new = B.Precond.multigrid3d_multi(op, 1, 0, kmax)
grids = new.multigrid_info()[1]
print(f"poisson {g}^3 on {op.variant()} / {op.spmm_variant()}, grids {grids}, nu 1, tol 1e-6", flush=True)
result["operator"], result["spmm"], result["grids"] = op.variant(), op.spmm_variant(), grids

print(f"{'k':>2} {'batched ms':>11} {'min':>8} {'max':>8} {'k singles ms':>13} {'min':>8} {'max':>8} {'speed-up':>9}  iterations (batched | single)")
for k in ks:
    def batched():
        _, _, stats = B.pcg_solve_multi(op, m, new, Bk[:k], X0[:k], max_iters=1000)
        assert all(s.converged == 1 for s in stats)
        return stats[0].time_total_ms, [s.iterations for s in stats]

    def singles():
        total, its = 0.0, []
        for j in range(k):
            _, _, st = B.pcg_solve_device(op, m, old, Bk[j], X0[j], max_iters=1000)
            assert st.converged == 1
            total += st.time_total_ms
            its.append(st.iterations)
        return total, its

    batched(), singles()  # warm-up
    tb, ts = [], []
    for _ in range(solves):
        t, ib = batched()
        tb.append(t)
        t, isg = singles()
        ts.append(t)
    rec = {"k": k, "batched_ms": spread(tb), "singles_ms": spread(ts), "iterations_batched": ib, "iterations_single": isg,
           "samples_batched": tb, "samples_singles": ts}
    rec["speedup"] = rec["singles_ms"]["median"] / rec["batched_ms"]["median"]
    rec["ranges_apart"] = rec["singles_ms"]["min"] > rec["batched_ms"]["max"]
    result["by_k"].append(rec)
    b_, s_ = rec["batched_ms"], rec["singles_ms"]
    print(f"{k:2d} {b_['median']:11.3f} {b_['min']:8.3f} {b_['max']:8.3f} {s_['median']:13.3f} {s_['min']:8.3f} {s_['max']:8.3f} {rec['speedup']:9.3f}  "
          f"{ib} | {isg}", flush=True)

# ---- 2. one application, wall time ----
result["application"] = []
r, z = B.DeviceVector(G, fill=1.0), B.DeviceVector(G, fill=0.0)
print(f"{'k':>2} {'block application ms':>21} {'k single applications ms':>25} {'ratio':>7}")
for k in ks:
    R, Z = B.DeviceVector(G * k, fill=1.0), B.DeviceVector(G * k, fill=0.0)
    new.apply_device_multi(op, k, R.ptr, Z.ptr)
    old.apply_device(op, r.ptr, z.ptr)
    wb, ws = [], []
    for _ in range(9):
        t0 = time.perf_counter()
        new.apply_device_multi(op, k, R.ptr, Z.ptr)
        wb.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(k):
            old.apply_device(op, r.ptr, z.ptr)
        ws.append((time.perf_counter() - t0) * 1e3)
    rec = {"k": k, "block_ms": spread(wb), "singles_ms": spread(ws)}
    rec["ratio"] = rec["singles_ms"]["median"] / rec["block_ms"]["median"]
    result["application"].append(rec)
    print(f"{k:2d} {rec['block_ms']['median']:21.3f} {rec['singles_ms']['median']:25.3f} {rec['ratio']:7.3f}   "
          f"(block {rec['block_ms']['min']:.3f} - {rec['block_ms']['max']:.3f}, singles {rec['singles_ms']['min']:.3f} - {rec['singles_ms']['max']:.3f})",
          flush=True)
    R.free(), Z.free()
r.free(), z.free()
old.destroy(), new.destroy()
op.free()

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
