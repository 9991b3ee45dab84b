"""The refusals the three single-vector preconditioned solves (spmv_amd_pcg_solve_device, spmv_amd_bicgstab_solve_device,
spmv_amd_gcr_solve_device) make before their first HIP call: the exact sentence of each, and which one wins. The checks are two
shared halves (csrc/single_solve.hpp) with each solver's own refusals between them, so every refusal is provoked in a call that also
holds EVERY LATER fault one call can hold: the sentence on stderr is the first one's, alone. Two faults cannot share a call: an
operator without run_device is a caller's table, "used before init" one of the library's (which all have run_device); and "not a
square system" needs an initialised operator, so it is left to the GPU tests. The calls run in a child process that has made no
other call into the library: nothing is initialised, and stderr is the library's alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

N = 9
SOLVERS = ("PCG", "BICGSTAB", "GCR")


def cases(tag):
    """(case, sentence) in the order of the checks; `case` names what the call is made of (the child's `call`)."""
    own = {"BICGSTAB": [("kind", "[BICGSTAB] preconditioner kind 'chebyshev' is built for symmetric definite matrices: BiCGSTAB takes "
                                 "'none' or 'jacobi': refused")],
           "GCR": [("restart", "[GCR] restart = -1: 1 .. 32, or 0 for the default 16: refused"),
                   ("kind", "[GCR] the preconditioner record is not one of this library's (unknown kind): refused")]}.get(tag, [])
    return ([("null", f"[{tag}] null argument"),
             ("run_device", f"[{tag}] operator 'mine' does not support the device-native interface"),
             ("max_iters", f"[{tag}] max_iters < 0")] + own +
            [("init", f"[{tag}] operator 'stencil5-csr' used before init"),
             ("rows", f"[{tag}] mat->rows < 1"),
             ("size", f"[{tag}] the preconditioner is for {N - 1} rows, mat->rows = {N}"),
             ("owner", "[PCG] the preconditioner was made from another operator: refused")])


def child():
    from conftest import load_binding

    B = load_binding()
    L = B._gcr_lib()
    L.spmv_amd_bicgstab_solve_device.argtypes = L.spmv_amd_pcg_solve_device.argtypes
    b, x = np.ones(N), np.zeros(N)
    st = B.CGStats()
    keep = []

    def call(tag, case):
        order = [c for c, _ in cases(tag)]
        at = order.index(case)
        later = lambda name: name in order and at <= order.index(name)  # the fault `name` is in this call: this case's or a later one's
        if later("run_device"):
            op = B.SpmvOperator()  # a caller's table
            op.name = b"mine"
            op = C.pointer(op)
        elif later("init"):
            op = B.Operator("stencil5-csr").op  # one of the library's, never initialised
        else:
            op = B.SpmvOperator()
            op.name = b"mine"
            op.run_device = B.RUN_DEVICE_FN(lambda dx, dy: 1)  # never called
            keep.append(op.run_device)
            op = C.pointer(op)
        cfg = B.CGConfig(-1 if later("max_iters") else 10, 1e-6, 0, 0)
        rows = 0 if later("rows") else N
        mat = B.HostMatrix(np.zeros(0, dtype=B.ENTRY_DTYPE), rows, rows, -1)
        # SpmvAmdPrecond (csrc/precond.hpp) begins: int kind; int n; const void* owner
        record = (C.c_int * 256)()
        bad_kind = {"BICGSTAB": 2, "GCR": 7}.get(tag)
        record[0] = bad_kind if bad_kind is not None and later("kind") else 1
        record[1] = N - 1 if later("size") else N
        record[2] = 16  # an owner that is no operator of the library
        args = [op, mat.ptr, C.cast(record, C.c_void_p), b.ctypes.data, x.ctypes.data, C.byref(cfg), None if later("null") else C.byref(st)]
        if tag == "GCR":
            args.insert(3, -1 if later("restart") else 0)
        entry = {"PCG": L.spmv_amd_pcg_solve_device, "BICGSTAB": L.spmv_amd_bicgstab_solve_device, "GCR": L.spmv_amd_gcr_solve_device}[tag]
        rc = entry(*args)
        os.write(2, f"== {tag} {case} {rc}\n".encode())

    for tag in SOLVERS:
        for case, _ in cases(tag):
            call(tag, case)
    assert np.all(x == 0.0)


def test_each_refusal_wins_over_every_later_one():
    here = os.path.abspath(__file__)
    out = subprocess.run([sys.executable, here], capture_output=True, text=True, timeout=300, cwd=os.path.dirname(here))
    assert out.returncode == 0, out.stderr
    said, lines = {}, []
    for line in out.stderr.splitlines():
        if line.startswith("== "):
            _, tag, case, rc = line.split()
            said[(tag, case)] = (int(rc), lines)
            lines = []
        else:
            lines.append(line)
    assert not lines, lines
    for tag in SOLVERS:
        for case, sentence in cases(tag):
            rc, got = said[(tag, case)]
            assert rc == 1 and got == [sentence], (tag, case, rc, got)
    assert len(said) == sum(len(cases(tag)) for tag in SOLVERS)


if __name__ == "__main__":
    child()
