"""The aggregation multigrid preconditioner measured (spmv_amd_precond_create_multigrid).
   python tools/multigrid_bench.py [--poisson 2000] [--headline 20000] [--solves 5] [--out FILE]
   python tools/multigrid_bench.py --cycle-trace [n=20000]     (the workload of measurement 1, to be run under a kernel trace)
1. --cycle-trace: on the synthetic n x n stencil, 10 SpMVs through run_device (stencil5_rowlds_kernel<0>) and 5 V(1, 1) cycles. Run it
   under `rocprofv3 --kernel-trace --stats -- python tools/multigrid_bench.py --cycle-trace` in a run of its own: the level-0 launch
   of residual_restrict_kernel is the longest of its launches, to be put beside the SpMV (model 58 / 56 bytes per row); the stats
   also give the launches per cycle and where a cycle's GPU time goes.
2. Time to solution on the Poisson stencil (centre 4, off -1), --poisson grid, b and x0 ~ N(0, 1) (seed = the grid), tol 1e-6:
   Jacobi-PCG and Chebyshev degree 4 (re-measured here) against multigrid nu = 0, 1, 2, alternated IN ONE PROCESS, 1 warm-up +
   --solves timed solves each; medians of time_total_ms, iterations, ratio to Jacobi.
3. The wall time of one application (spmv_amd_precond_apply_device, nu = 1, median of 9) on the Poisson grid and on each of its coarse
   grids down to 125 as a problem of its own: the differences are what each level of the cycle costs, launch cost included; beside it
   the launches of one cycle.
4. The --headline grid (synthetic +5 / -1, b = 1, x0 = 0: 14 CG iterations) at nu = 1 against Jacobi: the well-conditioned case, where
   multigrid is expected to lose or tie.
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


B.require_gpu()
B.lib().spmv_amd_set_device(0)

if "--cycle-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--cycle-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 20000
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0 and op.variant() == "stencil5/row-lds"
    pc = B.Precond.multigrid(op, 1)
    r, z = B.DeviceVector(n * n, fill=1.0), B.DeviceVector(n * n, fill=0.0)
    for _ in range(10):
        assert op.run_device(r, z) == 0
    B.lib().spmv_amd_device_synchronize()
    for _ in range(5):
        pc.apply_device(op, r.ptr, z.ptr)
    print(f"cycle-trace {n}^2: 10 run_device SpMVs, 5 V(1,1) cycles on grids {pc.multigrid_info()[1]}")
    pc.destroy()
    r.free(), z.free()
    op.free()
    sys.exit(0)

solves = opt("--solves", 5)
poisson_n = opt("--poisson", 2000)
headline_n = opt("--headline", 20000)
out_path = opt("--out", "")
result = {"solves": solves}


def alternate(op, m, pcs, b, x0, max_iters):
    """1 warm-up + `solves` timed solves of every preconditioner in turn; medians."""
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
        out[name] = {"iterations": its[name], "ms": med, "ms_per_iteration": med / its[name], "samples": ms[name]}
    for name in pcs:
        out[name]["ratio_to_jacobi"] = out[name]["ms"] / out["jacobi"]["ms"]
        print(f"{name:12s} iterations={out[name]['iterations']:6d} ms={out[name]['ms']:10.3f} ms/iteration={out[name]['ms_per_iteration']:.4f} "
              f"ratio to jacobi={out[name]['ratio_to_jacobi']:.3f}")
    return out


def poisson_entries(k):
    import scipy.sparse as sp

    t = sp.diags([np.full(k - 1, -1.0), np.full(k, 4.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = sp.coo_matrix(sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k)))
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row, A.col, A.data
    return e


def cycle_launches(grids, nu, rowlds_min_grid=512):
    """Launches of one V(nu, nu) cycle: a fused level takes one launch per step, every other level two."""
    total = 0
    for l, n in enumerate(grids):
        per_step = 1 if n >= rowlds_min_grid else 2
        if l == len(grids) - 1:
            total += 1 + 8 * per_step
        else:
            total += 1 + nu * per_step + 1 + 1 + (nu + 1) * per_step
    return total


# ---- 2. time to solution on the Poisson stencil ----
if poisson_n > 0:
    k = poisson_n
    m = B.HostMatrix(poisson_entries(k), k * k, k * k, k)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(k)
    b, x0 = rng.standard_normal(k * k), rng.standard_normal(k * k)
    pcs = {"jacobi": B.Precond(op, "jacobi"), "chebyshev4": B.Precond.chebyshev(op, 4)}
    for nu in (0, 1, 2):
        pcs[f"multigrid{nu}"] = B.Precond.multigrid(op, nu)
    grids = pcs["multigrid1"].multigrid_info()[1]
    print(f"poisson {k}^2 on {op.variant()}, grids {grids}")
    result["poisson"] = dict(alternate(op, m, pcs, b, x0, 100000), n=k, operator=op.variant(), grids=grids,
                             launches_per_cycle={nu: cycle_launches(grids, nu) for nu in (0, 1, 2)})
    print(f"launches per cycle: {result['poisson']['launches_per_cycle']}")
    for p in pcs.values():
        p.destroy()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()

    # ---- 3. one application on the grid and on each coarse grid as a problem of its own ----
    walls = {}
    for g in [g for g in grids if g >= 125]:
        mg = B.HostMatrix(poisson_entries(g), g * g, g * g, g)
        op = B.Operator("stencil5-csr")
        assert op.init(mg) == 0
        pc = B.Precond.multigrid(op, 1)
        r, z = B.DeviceVector(g * g, fill=1.0), B.DeviceVector(g * g, fill=0.0)
        pc.apply_device(op, r.ptr, z.ptr)
        samples = []
        for _ in range(9):
            t0 = time.perf_counter()
            pc.apply_device(op, r.ptr, z.ptr)
            samples.append((time.perf_counter() - t0) * 1e3)
        walls[g] = float(np.median(samples))
        print(f"one application from grid {g:5d} down: {walls[g]:.3f} ms wall, {cycle_launches(pc.multigrid_info()[1], 1)} launches")
        pc.destroy()
        r.free(), z.free()
        op.free()
        B.lib().spmv_amd_reset_host_matrices()
    result["application_wall_ms_from_grid"] = walls

# ---- 4. the headline matrix: where not to reach for it ----
if headline_n > 0:
    k = headline_n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(k) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), k * k, k * k, k)
    pcs = {"jacobi": B.Precond(op, "jacobi"), "multigrid1": B.Precond.multigrid(op, 1)}
    print(f"headline {k}^2 on {op.variant()}, grids {pcs['multigrid1'].multigrid_info()[1]}")
    result["headline"] = dict(alternate(op, m, pcs, np.ones(k * k), np.zeros(k * k), 1000), n=k, operator=op.variant())
    for p in pcs.values():
        p.destroy()
    op.free()

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
