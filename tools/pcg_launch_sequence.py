"""The kernel launches of ONE preconditioned solve, for comparing two builds of the library launch for launch.
   python tools/pcg_launch_sequence.py solve <operator> <grid> <none|jacobi|chebyshev:K|multigrid:NU> [--timers]
   python tools/pcg_launch_sequence.py list <..._kernel_trace.csv>
`solve` is the workload: the 5-point stencil (centre 5, off -1) on a grid x grid mesh in the named operator, b = 1, x0 = 0, tol 1e-6,
one solve between two marker launches (fill_kernel over 3 values). SPMV_AMD_LIB selects the library (binding.py). Run it under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pcg_launch_sequence.py solve ...`, a process of its own per
configuration, no other tracing or counters with it.
`list` prints what lies between the two markers of such a trace in launch order, one line per launch: kernel name, grid size,
workgroup size (template arguments kept, the anonymous namespace cut). Two builds launch the same sequence when the two lists are
equal line for line; profiles/r17_pcg_refactor_launch_sequence.txt holds such a comparison."""
import csv
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def solve(mode, n, kind, timers):
    import numpy as np

    spec = importlib.util.spec_from_file_location("spmv_amd_binding", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "binding.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    sys.path.insert(0, ROOT)
    from oracle import oracle as O

    B.require_gpu()
    B.lib().spmv_amd_set_device(0)
    rows = n * n
    m = B.HostMatrix(O.stencil5_coo(n), rows, rows, n)
    op = B.Operator(mode)
    assert op.init(m) == 0
    name, _, arg = kind.partition(":")
    if name == "chebyshev":
        pc = B.Precond.chebyshev(op, int(arg))
    elif name == "multigrid":
        pc = B.Precond.multigrid(op, int(arg))
    else:
        pc = B.Precond(op, name)
    marker = B.DeviceVector(3, fill=0.0)
    _, h, st = B.pcg_solve_device(op, m, pc, np.ones(rows), np.zeros(rows), timers=1 if timers else 0)
    B.lib().spmv_amd_device_fill_f64(marker.ptr, 3, 1.0)
    B.lib().spmv_amd_device_synchronize()
    assert st.converged == 1
    print(f"{mode} {n} {kind}{' --timers' if timers else ''}: variant {op.variant()}, {st.iterations} iterations, residual {h[-1]:.6e}")
    pc.destroy()
    marker.free()
    op.free()


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    out = []
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("spmv_amd::", "")
        name = name.split("(")[0].removeprefix("void ")
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        block = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        out.append(f"{name} grid {grid} workgroup {block}")
    marks = [i for i, line in enumerate(out) if line.startswith("fill_kernel ")]  # the solver launches none itself
    assert len(marks) >= 2, f"{path}: the two marker launches are not in the trace"
    return out[marks[-2] + 1:marks[-1]]


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "solve":
        solve(sys.argv[2], int(sys.argv[3]), sys.argv[4], "--timers" in sys.argv[5:])
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        print("\n".join(launches(sys.argv[2])))
    else:
        sys.exit(__doc__)
