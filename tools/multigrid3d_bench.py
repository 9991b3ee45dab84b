"""The aggregation multigrid preconditioner of the 3-D operator measured (spmv_amd_precond_create_multigrid3d).
   python tools/multigrid3d_bench.py [--grids 256,512] [--solves 5] [--out FILE]
   python tools/multigrid3d_bench.py --solve-trace [n=512]        (the workload of measurement 1, to be run under a kernel trace)
   python tools/multigrid3d_bench.py --kernel-summary <..._kernel_trace.csv> [--out FILE]
1. residual_restrict3d_kernel against the stencil7-csr SpMV and the r-update streaming kernel (pcg_update_r_kernel<false>, 24 B/row), all
   three in ONE process, alternated: --solve-trace runs multigrid-PCG solves (nu = 1) of the n^3 Poisson system, whose every iteration
   launches the three on level 0 one after the other. Run it under
   `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/multigrid3d_bench.py --solve-trace`, a process of its own, no
   other tracing or counters with it; --kernel-summary then takes each kernel's level-0 launches (its largest grid) out of the trace:
   median, min and max, the ratio to the SpMV (byte model 73 / 72 = 1.01) and the condition that fusing pays, restriction < SpMV +
   r-update.
2. Time to solution on the n^3 Poisson system (centre 6, neighbours -1, built on the device), b and x0 ~ N(0, 1) (seed = n), tol 1e-6:
   Jacobi-PCG and Chebyshev degree 4 against multigrid nu = 0, 1, 2, alternated in one process, 1 warm-up + --solves timed solves each;
   median with min and max of time_total_ms, iterations, ratio to Jacobi, the launches of one cycle, and whether multigrid nu = 1 is
   faster than Jacobi outside both ranges.
3. The wall time of one application (spmv_amd_precond_apply_device, nu = 1, median of 9) on the largest grid and on each of its coarse
   grids down to 64 as a problem of its own: what the levels of at most that grid cost inside the cycle, launch cost included.
Prints one line per measurement and a JSON summary (also written to --out)."""
import csv
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_summary(path):
    """Level-0 launches of the three kernels in a kernel trace: the launches of each kernel's largest grid."""
    kernels = {"spmv": "stencil7_rowlds_kernel<false>", "r_update": "pcg_update_r_kernel<false>", "residual_restrict3d": "residual_restrict3d_kernel"}
    found = {k: {} for k in kernels}
    for r in csv.DictReader(open(path)):
        for key, name in kernels.items():
            if name in r["Kernel_Name"]:
                us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                found[key].setdefault(int(r["Grid_Size_X"]), []).append(us)
    out = {}
    for key, by_grid in found.items():
        assert by_grid, f"{path}: no launch of {kernels[key]}"
        grid = max(by_grid)
        us = by_grid[grid]
        out[key] = {"kernel": kernels[key], "grid": grid, "launches": len(us), "median_us": float(np.median(us)), "min_us": min(us), "max_us": max(us)}
        print(f"{key:20s} grid {grid:10d} launches {len(us):4d} median {out[key]['median_us']:9.1f} us (min {min(us):.1f}, max {max(us):.1f})")
    rr, sp, ru = (out[k]["median_us"] for k in ("residual_restrict3d", "spmv", "r_update"))
    out["ratio_to_spmv"] = rr / sp
    out["byte_model_ratio"] = 73.0 / 72.0
    out["fusing_pays"] = bool(rr < sp + ru)
    print(f"residual_restrict3d / SpMV = {rr / sp:.3f} (byte model {73 / 72:.3f}); SpMV + r-update = {sp + ru:.1f} us: fusing pays = {out['fusing_pays']}")
    return out


if "--kernel-summary" in sys.argv:
    summary = kernel_summary(sys.argv[sys.argv.index("--kernel-summary") + 1])
    print(json.dumps(summary))
    if opt("--out", ""):
        with open(opt("--out", ""), "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0)

spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)
B.require_gpu()
B.lib().spmv_amd_set_device(0)


def poisson_operator(n):
    """stencil7-csr on the n^3 Poisson matrix built in HBM, and the host record the solver takes (sizes only)."""
    op = B.Operator("stencil7-csr")
    assert op.init_synthetic3d(n, 6.0, -1.0) == 0
    return op, B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), n ** 3, n ** 3, n)


if "--solve-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--solve-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 512
    op, m = poisson_operator(n)
    assert op.variant() == "stencil7/row-lds"
    pc = B.Precond.multigrid3d(op, 1)
    rng = np.random.default_rng(n)
    b, x0 = rng.standard_normal(n ** 3), rng.standard_normal(n ** 3)
    for _ in range(3):
        _, _, st = B.pcg_solve_device(op, m, pc, b, x0)
        assert st.converged == 1
    print(f"solve-trace {n}^3: 3 solves of {st.iterations} iterations, V(1,1) cycles on grids {pc.multigrid_info()[1]}")
    pc.destroy()
    op.free()
    sys.exit(0)

solves = opt("--solves", 5)
grids_arg = [int(g) for g in opt("--grids", "256,512").split(",")]
out_path = opt("--out", "")
result = {"solves": solves}


def alternate(op, m, pcs, b, x0, max_iters):
    """1 warm-up + `solves` timed solves of every preconditioner in turn; median, min and max."""
    def run(name):
        _, _, st = B.pcg_solve_device(op, m, pcs[name], b, x0, max_iters=max_iters)
        assert st.converged == 1, name
        return st.time_total_ms, st.iterations

    for name in pcs:
        run(name)
    ms, its = {name: [] for name in pcs}, {}
    for _ in range(solves):
        for name in pcs:
            t, its[name] = run(name)
            ms[name].append(t)
    out = {}
    for name in pcs:
        med = float(np.median(ms[name]))
        out[name] = {"iterations": its[name], "ms": med, "min_ms": min(ms[name]), "max_ms": max(ms[name]), "ms_per_iteration": med / its[name],
                     "samples": ms[name]}
    for name in pcs:
        out[name]["ratio_to_jacobi"] = out[name]["ms"] / out["jacobi"]["ms"]
        print(f"{name:12s} iterations={out[name]['iterations']:6d} ms={out[name]['ms']:10.3f} (min {out[name]['min_ms']:.3f}, max {out[name]['max_ms']:.3f}) "
              f"ms/iteration={out[name]['ms_per_iteration']:.4f} ratio to jacobi={out[name]['ratio_to_jacobi']:.3f}")
    return out


def cycle_launches(grids, nu):
    """Launches of one V(nu, nu) cycle: term 0, two launches per step (SpMV + streaming step), restriction and prolongation."""
    total = 0
    for l in range(len(grids)):
        total += 1 + 8 * 2 if l == len(grids) - 1 else 1 + nu * 2 + 1 + 1 + (nu + 1) * 2
    return total


for n in grids_arg:
    op, m = poisson_operator(n)
    rng = np.random.default_rng(n)
    b, x0 = rng.standard_normal(n ** 3), rng.standard_normal(n ** 3)
    pcs = {"jacobi": B.Precond(op, "jacobi"), "chebyshev4": B.Precond.chebyshev(op, 4)}
    for nu in (0, 1, 2):
        pcs[f"multigrid{nu}"] = B.Precond.multigrid3d(op, nu)
    grids = pcs["multigrid1"].multigrid_info()[1]
    print(f"poisson {n}^3 on {op.variant()}, grids {grids}")
    r = dict(alternate(op, m, pcs, b, x0, 100000), n=n, operator=op.variant(), grids=grids,
             launches_per_cycle={nu: cycle_launches(grids, nu) for nu in (0, 1, 2)})
    r["multigrid1_faster_than_jacobi_outside_both_ranges"] = bool(r["multigrid1"]["max_ms"] < r["jacobi"]["min_ms"])
    print(f"launches per cycle: {r['launches_per_cycle']}; multigrid nu = 1 faster than Jacobi outside both ranges: "
          f"{r['multigrid1_faster_than_jacobi_outside_both_ranges']} (factor {r['jacobi']['ms'] / r['multigrid1']['ms']:.2f})")
    result[f"poisson{n}"] = r
    for p in pcs.values():
        p.destroy()
    op.free()

# ---- 3. one application on the largest grid and on each coarse grid down to 64 as a problem of its own ----
walls = {}
top = max(grids_arg)
g = top
while g >= 64:
    op, m = poisson_operator(g)
    pc = B.Precond.multigrid3d(op, 1)
    rv, zv = B.DeviceVector(g ** 3, fill=1.0), B.DeviceVector(g ** 3, fill=0.0)
    pc.apply_device(op, rv.ptr, zv.ptr)
    samples = []
    for _ in range(9):
        t0 = time.perf_counter()
        pc.apply_device(op, rv.ptr, zv.ptr)
        samples.append((time.perf_counter() - t0) * 1e3)
    walls[g] = float(np.median(samples))
    print(f"one application from grid {g:4d}^3 down: {walls[g]:.3f} ms wall, {cycle_launches(pc.multigrid_info()[1], 1)} launches")
    pc.destroy()
    rv.free(), zv.free()
    op.free()
    g = (g + 1) // 2
result["application_wall_ms_from_grid"] = walls
if 64 in walls:
    result["share_of_levels_up_to_64"] = walls[64] / walls[top]
    print(f"levels of at most 64^3: {100 * walls[64] / walls[top]:.1f} % of one application from {top}^3")

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
