"""Batched AMG-preconditioned solves measured (spmv_amd_precond_create_amg_multi).
   python tools/amg_multi_bench.py [--poisson 2000] [--nine 1000] [--upwind 2000] [--ks 1,2,4,8] [--solves 5] [--out FILE]
   python tools/amg_multi_bench.py --restrict-trace [n=2000] [--ks 1,2,4,8]   (LAB build; to be run under a kernel trace)
1. --restrict-trace: on the n x n Poisson matrix held in cusparse-csr, level 0 of the AMG hierarchy, on the level's own arrays: for every
   k of --ks ten launches of amg_residual_restrict_multi_kernel<k> through spmv_amd_amg_multi_stage, and ten launches of the
   single-vector amg_residual_restrict_kernel through spmv_amd_amg_stage, in the same run. Run it under
   `rocprofv3 --kernel-trace --stats -- python tools/amg_multi_bench.py --restrict-trace` in a run of its own, no counters: the block
   launch's mean duration is to be put beside k times the single launch's. It prints the byte model from the level's measured
   aggregate count: per fine row of q entries 12 q + 12 shared plus 4 per aggregate, and per column 16 plus 8 per aggregate; the
   model's ratio at k is k * (shared + column) / (shared + k * column), the target 0.9 of it.
2. Time to solution at tol 1e-6, b_j ~ N(0, 1) (seed = the rows, then j), x0 = 0: ONE batched solve on k columns
   (spmv_amd_pcg_solve_device_multi on a handle of spmv_amd_precond_create_amg_multi) against k single solves
   (spmv_amd_pcg_solve_device on a handle of spmv_amd_precond_create_amg: the existing code, the baseline), alternated IN ONE PROCESS,
   1 warm-up + --solves timed rounds; medians of time_total_ms (the baseline: the sum over its k solves) with min - max. On the
   --poisson grid and the --nine grid (the 9-point stencil) in cusparse-csr; the same for GCR(16) on the --upwind grid of
   tools/gcr_bench.py's 5-point upwind convection-diffusion stencil in cusparse-csr. A grid of 0 skips its system.
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


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def entries_of(A):
    A = sp.coo_matrix(A)
    order = np.lexsort((A.col, A.row))
    e = np.zeros(A.nnz, dtype=B.ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = A.row[order], A.col[order], A.data[order]
    return e


def poisson(g):
    t = sp.diags([np.full(g - 1, -1.0), np.full(g, 4.0), np.full(g - 1, -1.0)], [-1, 0, 1])
    return sp.kron(sp.identity(g), t) + sp.kron(sp.diags([np.full(g - 1, -1.0), np.full(g - 1, -1.0)], [-1, 1]), sp.identity(g))


def ninepoint(g):
    band = sp.diags([np.ones(g - 1), np.ones(g), np.ones(g - 1)], [-1, 0, 1])
    return 9.0 * sp.identity(g * g) - sp.kron(band, band)


def upwind(g):
    px, py = 2.0, 0.5
    t = sp.diags([np.full(g - 1, -1.0 - px), np.full(g, 4.0 + px + py), np.full(g - 1, -1.0)], [-1, 0, 1])
    return sp.kron(sp.identity(g), t) + sp.kron(sp.diags([np.full(g - 1, -1.0 - py), np.full(g - 1, -1.0)], [-1, 1]), sp.identity(g))


ks = [int(v) for v in opt("--ks", "1,2,4,8").split(",")]

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
    kmax = max(ks)
    z, r, rc = B.DeviceVector(rows * kmax, fill=1.0), B.DeviceVector(rows * kmax, fill=0.5), B.DeviceVector(coarse * kmax, fill=0.0)
    a = B.AmgStageArgs(rows=rows, cols=rows, coarse_rows=coarse, row_ptr=held[0].ptr, col_idx=held[1].ptr, values=held[2].ptr,
                       agg_ptr=held[3].ptr, members=held[4].ptr, z=z.ptr, r=r.ptr, coarse=rc.ptr)
    for _ in range(10):
        assert B.amg_stage("residual_restrict", a) == 0
    for k in ks:
        for _ in range(10):
            assert B.amg_multi_stage("residual_restrict", k, a) == 0
    B.lib().spmv_amd_device_synchronize()
    q, per_row = len(ci) / rows, coarse / rows
    shared, column = 12 * q + 12 + 4 * per_row, 16 + 8 * per_row
    print(f"restrict-trace {n}^2 on {op.variant()}: level rows {info['rows']}, {coarse} aggregates ({per_row:.4f} per fine row), "
          f"{q:.3f} entries per row: shared {shared:.2f} B, per column {column:.2f} B per fine row")
    for k in ks:
        model = k * (shared + column) / (shared + k * column)
        print(f"k={k}: block launch {(shared + k * column) * rows / 1e6:.1f} MB, k single launches {k * (shared + column) * rows / 1e6:.1f} MB, "
              f"model ratio {model:.3f}, target {0.9 * model:.3f}")
    pc.destroy()
    op.free()
    sys.exit(0)

B.require_gpu()
B.lib().spmv_amd_set_device(0)
solves = opt("--solves", 5)
out_path = opt("--out", "")
result = {"solves": solves, "tol": 1e-6, "nu": 1, "systems": {}}


def measure(label, A, g, gcr):
    rows = g * g
    B.lib().spmv_amd_reset_host_matrices()
    m = B.HostMatrix(entries_of(A), rows, rows, -1)
    op = B.Operator("cusparse-csr")
    assert op.init(m) == 0
    kmax = max(ks)
    Bk = np.stack([np.random.default_rng([rows, j]).standard_normal(rows) for j in range(kmax)])
    X0 = np.zeros((kmax, rows))
    old, new = B.Precond.amg(op, 1), B.Precond.amg_multi(op, 1, 0, 0.08, kmax)
    info = new.amg_info()
    solver = "GCR(16)" if gcr else "PCG"
    print(f"{label} {g}^2 on {op.variant()} / {op.spmm_variant()}, {solver}, AMG nu 1: level rows {info['rows']}, set-up {info['setup_ms']:.1f} ms "
          f"(single handle {old.amg_info()['setup_ms']:.1f} ms)", flush=True)
    out = {"n": g, "solver": solver, "operator": op.variant(), "spmm": op.spmm_variant(), "level_rows": info["rows"], "by_k": []}
    print(f"{'k':>2} {'batched ms':>11} {'min':>8} {'max':>8} {'k singles ms':>13} {'min':>8} {'max':>8} {'speed-up':>9}  iterations (batched | single)")
    for k in ks:
        def batched():
            if gcr:
                _, _, stats = B.gcr_solve_multi(op, m, new, Bk[:k], X0[:k], restart=16, max_iters=1000)
            else:
                _, _, stats = B.pcg_solve_multi(op, m, new, Bk[:k], X0[:k], max_iters=1000)
            assert all(s.converged == 1 for s in stats)
            return stats[0].time_total_ms, [s.iterations for s in stats]

        def singles():
            total, its = 0.0, []
            for j in range(k):
                if gcr:
                    _, _, st = B.gcr_solve(op, m, old, Bk[j], X0[j], restart=16, max_iters=1000)
                else:
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
        rec["ranges_apart"] = rec["singles_ms"]["min"] > rec["batched_ms"]["max"] or rec["batched_ms"]["min"] > rec["singles_ms"]["max"]
        out["by_k"].append(rec)
        b_, s_ = rec["batched_ms"], rec["singles_ms"]
        print(f"{k:2d} {b_['median']:11.3f} {b_['min']:8.3f} {b_['max']:8.3f} {s_['median']:13.3f} {s_['min']:8.3f} {s_['max']:8.3f} "
              f"{rec['speedup']:9.3f}  {ib} | {isg}", flush=True)
    old.destroy(), new.destroy()
    op.free()
    return out


for name, make, flag, default, gcr in (("poisson", poisson, "--poisson", 2000, False), ("ninepoint", ninepoint, "--nine", 1000, False),
                                       ("upwind", upwind, "--upwind", 2000, True)):
    g = opt(flag, default)
    if g > 0:
        result["systems"][name] = measure(name, make(g), g, gcr)
B.lib().spmv_amd_reset_host_matrices()
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
