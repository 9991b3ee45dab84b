"""Batched multigrid-preconditioned CG measured (spmv_amd_precond_create_multigrid_multi).
   python tools/mg_multi_bench.py [--poisson 2000] [--ks 1,2,4,8] [--solves 5] [--out FILE]
   python tools/mg_multi_bench.py --cycle-trace [n=20000] [--k 4] [--check]   (to be run under a kernel trace)
1. Time to solution on the Poisson stencil (centre 4, off -1), --poisson grid, nu = 1, tol 1e-6, k right-hand sides b_j ~ N(0, 1) from
   x0 ~ N(0, 1) (seed = the grid; column 0 is tools/multigrid_bench.py's system): ONE batched solve
   (spmv_amd_pcg_solve_device_multi on a handle of spmv_amd_precond_create_multigrid_multi) against k single-RHS solves
   (spmv_amd_pcg_solve_device on a handle of spmv_amd_precond_create_multigrid: the existing code, the baseline), alternated IN ONE
   PROCESS, 1 warm-up + --solves timed rounds; medians of time_total_ms (the baseline: the sum over its k solves) with min - max.
   Model, per cycle and system: restriction (40 + 18 k) / k against 58 bytes per fine row, a smoothing step
   (40 + 64 k) / k against 88, and the launch cost of the small levels divided by k.
2. The wall time of one application (nu = 1, median of 9): spmv_amd_precond_apply_device_multi on k columns against k calls of
   spmv_amd_precond_apply_device. Both synchronise; the model divides section 15's launch share (0.234 of 0.644 ms at 2 000^2) by k.
3. --cycle-trace: on the synthetic n x n stencil, 3 single-vector V(1, 1) cycles and 3 cycles on --k columns. Run it under
   `rocprofv3 --kernel-trace --stats -- python tools/mg_multi_bench.py --cycle-trace` in a run of its own (no counters): the level-0
   launch of residual_restrict_multi_kernel<k> is to be put beside k launches of residual_restrict_kernel. --check downloads column 0
   of the block result and compares it with the single-vector result bit for bit.
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


B.require_gpu()
B.lib().spmv_amd_set_device(0)

if "--cycle-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--cycle-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 20000
    k = opt("--k", 4)
    N = n * n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0 and op.variant() == "stencil5/row-lds"
    pc = B.Precond.multigrid_multi(op, 1, 0, k)
    r, z = B.DeviceVector(N, fill=1.0), B.DeviceVector(N, fill=0.0)
    R, Z = B.DeviceVector(N * k, fill=1.0), B.DeviceVector(N * k, fill=0.0)
    for _ in range(3):
        pc.apply_device(op, r.ptr, z.ptr)
    for _ in range(3):
        pc.apply_device_multi(op, k, R.ptr, Z.ptr)
    print(f"cycle-trace {n}^2: 3 single V(1,1) cycles, 3 cycles on {k} columns, grids {pc.multigrid_info()[1]}")
    if "--check" in sys.argv:
        single = z.to_host()
        block = Z.to_host().reshape(N, k)
        same = all(np.array_equal(single.view(np.uint64), np.ascontiguousarray(block[:, j]).view(np.uint64)) for j in range(k))
        print(f"every column of the block result equals the single-vector result bit for bit: {same}")
        assert same
    pc.destroy()
    for v in (r, z, R, Z):
        v.free()
    op.free()
    sys.exit(0)

solves = opt("--solves", 5)
g = opt("--poisson", 2000)
ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]
out_path = opt("--out", "")
result = {"solves": solves, "n": g, "nu": 1, "tol": 1e-6, "by_k": []}


def poisson_entries(k):
    import scipy.sparse as sp

    t = sp.diags([np.full(k - 1, -1.0), np.full(k, 4.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = sp.coo_matrix(sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k)))
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row, A.col, A.data
    return e


G = g * g
m = B.HostMatrix(poisson_entries(g), G, G, g)
op = B.Operator("stencil5-csr")
assert op.init(m) == 0
kmax = max(ks)
rng = np.random.default_rng(g)
Bk = np.empty((kmax, G))
X0 = np.empty((kmax, G))
for j in range(kmax):  # column 0: b, then x0, as tools/multigrid_bench.py draws them
    Bk[j], X0[j] = rng.standard_normal(G), rng.standard_normal(G)
old = B.Precond.multigrid(op, 1)
new = B.Precond.multigrid_multi(op, 1, 0, kmax)
grids = new.multigrid_info()[1]
print(f"poisson {g}^2 on {op.variant()} / {op.spmm_variant()}, grids {grids}, nu 1, tol 1e-6", flush=True)
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
