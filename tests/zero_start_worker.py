"""One rank of tests/test_zero_start_gpu.py's slab with neighbours: WORLD_SIZE processes sharing the GPU over the staged / gloo
communicator (as tests/dist_worker.py, mode gpu-synthetic), on the LAB build. Usage: zero_start_worker.py N, with RANK, WORLD_SIZE,
MASTER_ADDR and MASTER_PORT in the environment."""
import datetime
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
from conftest import load_binding, hist_err  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(n, rank, world):
    B = load_binding().use_lab()
    B.lib()
    comm = B.Comm.staged_over_torch(rank, world, dist)
    N = n * n
    slab = B.CgSlab.stencil5(n, comm)
    # a row-lds slab in ring mode, whose first SpMV writes the residual: on one rank it would take both forms, so form 0 below can
    # only come from the gate on neighbours
    assert slab.variant() == "stencil5/row-lds" and "in-place" not in slab.loop_shape(), (slab.variant(), slab.loop_shape())
    runs = []
    for value in (0, 1, 0, 1):
        slab.set_option("zero_start", value)
        assert slab.initial_form() == 0  # neither form: the first launch of a slab with neighbours reads x0 and its halo rows
        st = slab.solve()
        runs.append((st.iterations, st.converged, slab.history().copy(), slab.gather()))
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and np.array_equal(bits(r[2]), bits(runs[0][2])) and np.array_equal(bits(r[3]), bits(runs[0][3]))
    if rank == 0:
        rp, ci, va = O.stencil5_csr(n)
        xo, ho, ro = O.cg_partitioned(rp, ci, va, n, np.ones(N), np.zeros(N), world=world)
        assert runs[0][:2] == (ro.iterations, 1) and hist_err(runs[0][2], ho) < 1e-10
        assert np.max(np.abs(runs[0][3] - xo)) <= 1e-10 * np.max(np.abs(xo))
    slab.destroy()
    comm.destroy()
    print(f"rank {rank}: zero start on a slab with neighbours ok")


def main():
    n = int(sys.argv[1])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        run(n, rank, world)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
