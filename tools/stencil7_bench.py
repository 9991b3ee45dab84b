"""The 3-D operator measured (stencil7-csr).
   python tools/stencil7_bench.py [--sizes 64,96,128,160,256,512,640] [--cg 512] [--out-dir profiles]
One process per size (the parent starts them one after the other and collects their JSON lines). Inside a size the kernels are
ALTERNATED -- stencil7/row-lds, stencil7/row-direct and, from 256^3 up, cusparse-csr (csr/stream) on the same device-generated
matrix -- through spmv_amd_time_run_device on the operators' own vectors (x = 1): one untimed round, then --rounds rounds of --reps
launches each, every launch timed with events. Reported per kernel: median, min, max in ms, GB/s and the fraction of 8 TB/s by the
72 B/row model (8 nnz + 16 rows), and the ratio to csr/stream.
At 512^3 and 640^3 the same process then sweeps the XCD run length of row-lds (SPMV_AMD_ROWLDS_GROUP, re-read when the variant is
selected): 1, tiles per grid row, twice that, the 2-D rule rowlds_xcd_run_rule(n), tiles per plane / 8 capped at 64.
--cg N: cg_solve_device on the generator matrix (b = 1, x0 = 0, tol 1e-6), stencil7-csr against cusparse-csr, alternated, one
untimed and five timed solves each: iterations, ms per iteration.
Writes <out-dir>/r18_stencil7_bench.txt and .json. Loads the LAB build, like the other tools."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12  # B/s, MI355X HBM3E


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def binding():
    spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lab = mod.use_lab()
    lab.require_gpu()
    lab.lib().spmv_amd_set_device(0)
    return lab


def summary(samples, model_bytes):
    s = np.sort(np.asarray(samples, dtype=np.float64))
    med = float(np.median(s))
    return {"ms": med, "min_ms": float(s[0]), "max_ms": float(s[-1]), "gbs": model_bytes / med / 1e6, "fraction_of_peak": model_bytes / (med * 1e-3) / PEAK,
            "samples": len(s)}


def alternate(kernels, rounds, reps, model_bytes):
    """kernels: name -> callable returning `reps` launch times; one untimed round first"""
    for run in kernels.values():
        run(reps)
    samples = {name: [] for name in kernels}
    for _ in range(rounds):
        for name, run in kernels.items():
            samples[name].extend(run(reps))
    return {name: summary(v, model_bytes) for name, v in samples.items()}


def child_size(n, rounds, reps):
    B = binding()
    N, nnz = n ** 3, 7 * n ** 3 - 6 * n ** 2
    model = 8.0 * nnz + 16.0 * N
    s7 = B.Operator("stencil7-csr")
    assert s7.init_synthetic3d(n) == 0
    out = {"n": n, "rows": N, "nnz": nnz, "model_bytes": model, "auto": s7.variant(), "placement": s7.placement()}

    def forced(variant):
        def run(k):
            assert s7.select_variant(variant) == 0 and s7.variant() == "stencil7/" + variant
            return list(s7.time_device(None, None, k))
        return run

    kernels = {"stencil7/row-lds": forced("row-lds"), "stencil7/row-direct": forced("row-direct")}
    csr = None
    if n >= 256:
        csr = B.Operator("cusparse-csr")
        assert csr.init_synthetic3d(n) == 0 and csr.variant() == "csr/stream"
        kernels["csr/stream"] = lambda k: list(csr.time_device(None, None, k))
    out["kernels"] = alternate(kernels, rounds, reps, model)
    if csr is not None:
        for name in kernels:
            out["kernels"][name]["ratio_to_csr_stream"] = out["kernels"]["csr/stream"]["ms"] / out["kernels"][name]["ms"]
        csr.free()
    if n >= 512:
        tiles = (n + 127) // 128
        rule_2d = 4 if n < 8000 else max(1, min(64, int(1.05 * tiles / 8.0 + 0.5)))  # rowlds_xcd_run_rule(n), csrc/spmv_kernels.hip
        runs = sorted({1, tiles, 2 * tiles, rule_2d, min(64, tiles * n // 8)})

        def with_run(r):
            def run(k):
                os.environ["SPMV_AMD_ROWLDS_GROUP"] = str(r)
                assert s7.select_variant("row-lds") == 0
                return list(s7.time_device(None, None, k))
            return run

        out["xcd_run"] = alternate({str(r): with_run(r) for r in runs}, rounds, reps, model)
        os.environ.pop("SPMV_AMD_ROWLDS_GROUP", None)
    s7.select_variant(None)
    s7.free()
    print("RESULT " + json.dumps(out), flush=True)


def child_cg(n, solves):
    B = binding()
    N = n ** 3
    # the matrix is generated on the device: cg_solve_device reads only the row count of the MatrixData it is handed
    m = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), N, N, n)
    b, x0 = np.ones(N), np.zeros(N)
    ops = {}
    for mode in ("stencil7-csr", "cusparse-csr"):
        ops[mode] = B.Operator(mode)
        assert ops[mode].init_synthetic3d(n) == 0
    out = {"n": n, "rows": N, "variants": {mode: op.variant() for mode, op in ops.items()}}
    ms, its = {mode: [] for mode in ops}, {}
    for k in range(solves + 1):
        for mode, op in ops.items():
            _, hist, st = B.cg_solve(op, m, b, x0, max_iters=1000, tol=1e-6, device=True)
            assert st.converged == 1
            its[mode] = st.iterations
            if k > 0:
                ms[mode].append(st.time_total_ms)
    for mode in ops:
        med = float(np.median(ms[mode]))
        out[mode] = {"iterations": its[mode], "ms": med, "min_ms": min(ms[mode]), "max_ms": max(ms[mode]), "ms_per_iteration": med / its[mode]}
        ops[mode].free()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args):
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
    if done.returncode != 0 or not lines:
        raise RuntimeError(f"child {args} failed ({done.returncode}):\n{done.stdout[-3000:]}")
    return json.loads(lines[-1][len("RESULT "):])


def main():
    rounds, reps = opt("--rounds", 4), opt("--reps", 5)
    if "--child-size" in sys.argv:
        return child_size(opt("--child-size", 0), rounds, reps)
    if "--child-cg" in sys.argv:
        return child_cg(opt("--child-cg", 0), opt("--solves", 5))
    sizes = [int(s) for s in opt("--sizes", "64,96,128,160,256,512,640").split(",") if s]
    cg_n, out_dir = opt("--cg", 512), opt("--out-dir", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    result = {"rounds": rounds, "reps": reps, "sizes": [], "cg": None}
    text = [f"stencil7 bench: {rounds} rounds x {reps} launches per kernel, alternated, one untimed round first; model 72 B/row = 8 nnz + 16 rows; peak 8 TB/s"]
    for n in sizes:
        r = run_child(["--child-size", str(n), "--rounds", str(rounds), "--reps", str(reps)])
        result["sizes"].append(r)
        text.append(f"\n{n}^3: {r['rows']} rows, {r['nnz']} nnz, auto = {r['auto']}, y placement (candidates, gain) = {r['placement']}")
        for name, k in r["kernels"].items():
            ratio = f"  x csr/stream {k['ratio_to_csr_stream']:.3f}" if "ratio_to_csr_stream" in k else ""
            text.append(f"  {name:20s} median {k['ms']:9.4f} ms  min {k['min_ms']:9.4f}  max {k['max_ms']:9.4f}  {k['gbs']:8.1f} GB/s  "
                        f"{k['fraction_of_peak']:.3f} of peak{ratio}")
        for run, k in r.get("xcd_run", {}).items():
            text.append(f"  row-lds, XCD run {run:>3s}   median {k['ms']:9.4f} ms  min {k['min_ms']:9.4f}  max {k['max_ms']:9.4f}  {k['fraction_of_peak']:.3f} of peak")
        print("\n".join(text[-(2 + len(r["kernels"]) + len(r.get("xcd_run", {}))):]), flush=True)
    if cg_n > 0:
        c = run_child(["--child-cg", str(cg_n)])
        result["cg"] = c
        text.append(f"\ncg_solve_device at {cg_n}^3 (generator matrix, b = 1, x0 = 0, tol 1e-6), alternated, 5 timed solves each:")
        for mode in ("stencil7-csr", "cusparse-csr"):
            k = c[mode]
            text.append(f"  {mode:14s} ({c['variants'][mode]}) iterations {k['iterations']}  median {k['ms']:.3f} ms  min {k['min_ms']:.3f}  max {k['max_ms']:.3f}  "
                        f"{k['ms_per_iteration']:.4f} ms/iteration")
        print("\n".join(text[-3:]), flush=True)
    with open(os.path.join(out_dir, "r18_stencil7_bench.txt"), "w") as f:
        f.write("\n".join(text) + "\n")
    with open(os.path.join(out_dir, "r18_stencil7_bench.json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
