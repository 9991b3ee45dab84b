"""The Chebyshev polynomial preconditioner measured (spmv_amd_precond_create_chebyshev).
   python tools/chebyshev_bench.py [--poisson 2000] [--headline 20000] [--solves 5] [--out FILE]
   python tools/chebyshev_bench.py --step-trace [n=20000]     (the workload of measurement 1, to be run under a kernel trace)
1. --step-trace: on the synthetic n x n stencil, 10 SpMVs through run_device (stencil5_rowlds_kernel<0>) and 5 applications of
   degree 4 (20 launches of the fused step, stencil5_rowlds_kernel<3>). Run it under `rocprofv3 --kernel-trace --stats -- python
   tools/chebyshev_bench.py --step-trace` in a run of its own and divide the two kernels' average durations: model 88 / 56 = 1.57.
2. Time to solution on the Poisson stencil (centre 4, off -1), --poisson grid, b and x0 ~ N(0, 1) (seed = the grid), tol 1e-6:
   Jacobi-PCG against Chebyshev of degrees 2, 4 and 8, alternated IN ONE PROCESS, 1 warm-up + --solves timed solves each; medians
   of time_total_ms, iterations, ratio to Jacobi. Byte model (144 + 88 k against 136 per row and iteration): about 0.83 at degrees
   2 and 4.
3. The --headline grid (synthetic +5 / -1, b = 1, x0 = 0: 14 CG iterations) at degree 4 against Jacobi, the same way: the
   well-conditioned case, where the polynomial is expected to lose (about 1.5x by bytes).
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


B.require_gpu()
B.lib().spmv_amd_set_device(0)

if "--step-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--step-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 20000
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(n) == 0 and op.variant() == "stencil5/row-lds"
    pc = B.Precond.chebyshev(op, 4)
    r, z = B.DeviceVector(n * n, fill=1.0), B.DeviceVector(n * n, fill=0.0)
    for _ in range(10):
        assert op.run_device(r, z) == 0
    B.lib().spmv_amd_device_synchronize()
    for _ in range(5):
        pc.apply_device(op, r.ptr, z.ptr)
    print(f"step-trace {n}^2: 10 run_device SpMVs, 5 applications of degree 4")
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


# ---- 2. time to solution on the Poisson stencil ----
if poisson_n > 0:
    import scipy.sparse as sp

    k = poisson_n
    t = sp.diags([np.full(k - 1, -1.0), np.full(k, 4.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = sp.coo_matrix(sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k)))
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row, A.col, A.data
    m = B.HostMatrix(e, k * k, k * k, k)
    op = B.Operator("stencil5-csr")
    assert op.init(m) == 0
    rng = np.random.default_rng(k)
    b, x0 = rng.standard_normal(k * k), rng.standard_normal(k * k)
    pcs = {"jacobi": B.Precond(op, "jacobi")}
    for degree in (2, 4, 8):
        pcs[f"chebyshev{degree}"] = B.Precond.chebyshev(op, degree)
    print(f"poisson {k}^2 on {op.variant()}, interval {pcs['chebyshev4'].chebyshev_info()[1:3]}")
    result["poisson"] = dict(alternate(op, m, pcs, b, x0, 100000), n=k, operator=op.variant())
    for p in pcs.values():
        p.destroy()
    op.free()
    B.lib().spmv_amd_reset_host_matrices()

# ---- 3. the headline matrix: where not to reach for it ----
if headline_n > 0:
    k = headline_n
    op = B.Operator("stencil5-csr")
    assert op.init_synthetic(k) == 0
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), k * k, k * k, k)
    pcs = {"jacobi": B.Precond(op, "jacobi"), "chebyshev4": B.Precond.chebyshev(op, 4)}
    print(f"headline {k}^2 on {op.variant()}")
    result["headline"] = dict(alternate(op, m, pcs, np.ones(k * k), np.zeros(k * k), 1000), n=k, operator=op.variant())
    for p in pcs.values():
        p.destroy()
    op.free()

print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
