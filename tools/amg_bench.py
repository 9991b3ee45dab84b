"""The aggregation AMG preconditioner measured (spmv_amd_precond_create_amg).
   python tools/amg_bench.py [--poisson 2000] [--nine 1000] [--solves 5] [--out FILE]
   python tools/amg_bench.py --restrict-trace [n=2000]     (the workload of measurement 1, to be run under a kernel trace)
1. --restrict-trace (LAB build): on the n x n Poisson matrix held in cusparse-csr, level 0 of the AMG hierarchy: 10 launches of
   amg_residual_restrict_kernel through spmv_amd_amg_stage on the level's own arrays, 10 products through run_device (the level's
   launch_csr_spmv) and 10 streaming r updates (spmv_amd_blas1_axpy). Run it under
   `rocprofv3 --kernel-trace --stats -- python tools/amg_bench.py --restrict-trace` in a run of its own, no counters: the three
   kernels' mean durations are the figures; the byte model per fine row of q entries is 12 q + 28 + 8 gathered.
2. Time to solution at tol 1e-6, b ~ N(0, 1) (seed = the rows), x0 = 0, alternated IN ONE PROCESS, 1 warm-up + --solves timed solves
   each, medians with ranges: the --poisson grid in cusparse-csr under Jacobi and AMG nu = 1, and in stencil5-csr under the
   geometric multigrid nu = 1; the --nine grid (the 9-point stencil, which the geometric creator refuses) in cusparse-csr under Jacobi
   and AMG nu = 1.
3. Set-up time (spmv_amd_precond_amg_info's setup_ms: host wall time of the whole creation) and the levels of both matrices.
Prints one line per measurement and a JSON summary (also written to --out)."""
import importlib.util
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def entries_of(A):
    A = sp.coo_matrix(A)
    order = np.lexsort((A.col, A.row))
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row[order], A.col[order], A.data[order]
    return e


def poisson(k):
    t = sp.diags([np.full(k - 1, -1.0), np.full(k, 4.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    return sp.kron(sp.identity(k), t) + sp.kron(sp.diags([np.full(k - 1, -1.0), np.full(k - 1, -1.0)], [-1, 1]), sp.identity(k))


def ninepoint(k):
    band = sp.diags([np.ones(k - 1), np.ones(k), np.ones(k - 1)], [-1, 0, 1])
    return 9.0 * sp.identity(k * k) - sp.kron(band, band)


if "--restrict-trace" in sys.argv:
    rest = sys.argv[sys.argv.index("--restrict-trace") + 1:]
    n = int(rest[0]) if rest and not rest[0].startswith("--") else 2000
    B = B.use_lab()
    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    rows = n * n
    op = B.Operator("cusparse-csr")
    assert op.init(B.HostMatrix(entries_of(poisson(n)), rows, rows, -1)) == 0
    pc = B.Precond.amg(op, 1)
    info = pc.amg_info()
    rp, ci, va, _, agg = pc.amg_level(0)
    members = np.argsort(agg, kind="stable").astype(np.int32)
    coarse = info["rows"][1]
    agg_ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=coarse))]).astype(np.int32)

    def on_device(a):
        a = np.ascontiguousarray(a)
        v = B.DeviceVector((a.nbytes + 7) // 8)
        B.lib().spmv_amd_copy_to_device(v.ptr, a.ctypes.data, a.nbytes)
        return v

    held = [on_device(a) for a in (rp, ci, va, agg_ptr, members)]
    z, r, w, rc = B.DeviceVector(rows, fill=1.0), B.DeviceVector(rows, fill=0.5), B.DeviceVector(rows, fill=0.0), B.DeviceVector(coarse, fill=0.0)
    a = B.AmgStageArgs(rows=rows, cols=rows, coarse_rows=coarse, row_ptr=held[0].ptr, col_idx=held[1].ptr, values=held[2].ptr,
                       agg_ptr=held[3].ptr, members=held[4].ptr, z=z.ptr, r=r.ptr, coarse=rc.ptr)
    for _ in range(10):
        assert B.amg_stage("residual_restrict", a) == 0
    for _ in range(10):
        assert op.run_device(z, w) == 0
        assert B.lib().spmv_amd_blas1_axpy(rows, -1.0, w.ptr, r.ptr) == 0
    B.lib().spmv_amd_device_synchronize()
    q = len(ci) / rows
    print(f"restrict-trace {n}^2 on {op.variant()}: level rows {info['rows']}, largest aggregates {info['max_aggregate']}, "
          f"{q:.2f} entries per row: byte model {12 * q + 28 + 8:.1f} B per fine row ({(12 * q + 36) * rows / 1e6:.1f} MB a launch)")
    pc.destroy()
    op.free()
    sys.exit(0)

B.require_gpu()
B.lib().spmv_amd_set_device(0)
solves = opt("--solves", 5)
out_path = opt("--out", "")
result = {"solves": solves}


def alternate(runs):
    """runs: name -> a function that solves once and returns (time_total_ms, iterations). 1 warm-up + `solves` timed solves of each
    in turn; medians with ranges."""
    for run in runs.values():
        run()
    ms, its = {name: [] for name in runs}, {}
    for _ in range(solves):
        for name, run in runs.items():
            t, its[name] = run()
            ms[name].append(t)
    out = {}
    for name in runs:
        med = float(np.median(ms[name]))
        out[name] = {"iterations": its[name], "ms": med, "min_ms": min(ms[name]), "max_ms": max(ms[name]), "samples": ms[name]}
    for name in runs:
        out[name]["ratio_to_jacobi"] = out[name]["ms"] / out["jacobi"]["ms"]
        print(f"{name:22s} iterations={out[name]['iterations']:6d} ms={out[name]['ms']:10.3f} [{out[name]['min_ms']:.3f}, {out[name]['max_ms']:.3f}] "
              f"ratio to jacobi={out[name]['ratio_to_jacobi']:.3f}")
    return out


def solver(op, m, pc, b, x0):
    def run():
        _, _, st = B.pcg_solve_device(op, m, pc, b, x0, max_iters=100000)
        assert st.converged == 1
        return st.time_total_ms, st.iterations
    return run


def measure(label, A, k, grid):
    rows = k * k
    e = entries_of(A)
    rng = np.random.default_rng(rows)
    b, x0 = rng.standard_normal(rows), np.zeros(rows)
    m = B.HostMatrix(e, rows, rows, -1)
    csr = B.Operator("cusparse-csr")
    assert csr.init(m) == 0
    held = [B.Precond(csr, "jacobi"), B.Precond.amg(csr, 1)]
    info = held[1].amg_info()
    print(f"{label} {k}^2 on {csr.variant()}: set-up {info['setup_ms']:.1f} ms, level rows {info['rows']}, entries {info['nnz']}, "
          f"largest aggregates {info['max_aggregate']}")
    runs = {"jacobi": solver(csr, m, held[0], b, x0), "amg1": solver(csr, m, held[1], b, x0)}
    stencil = None
    if grid:
        mg = B.HostMatrix(e, rows, rows, k)
        stencil = B.Operator("stencil5-csr")
        assert stencil.init(mg) == 0
        held.append(B.Precond.multigrid(stencil, 1))
        runs["geometric1 (stencil5-csr)"] = solver(stencil, mg, held[2], b, x0)
    out = dict(alternate(runs), n=k, operator=csr.variant(), setup_ms=info["setup_ms"], level_rows=info["rows"], level_nnz=info["nnz"],
               max_aggregate=info["max_aggregate"])
    for p in held:
        p.destroy()
    csr.free()
    if stencil is not None:
        stencil.free()
    B.lib().spmv_amd_reset_host_matrices()
    return out


poisson_n, nine_n = opt("--poisson", 2000), opt("--nine", 1000)
if poisson_n > 0:
    result["poisson"] = measure("poisson", poisson(poisson_n), poisson_n, True)
if nine_n > 0:
    result["ninepoint"] = measure("9-point", ninepoint(nine_n), nine_n, False)
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
