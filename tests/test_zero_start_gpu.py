"""The two ends of a solve on a slab without neighbours that owns its matrix (csrc/slab_decisions.hpp LoopShape::zero_start, r0_in_ring and
x0_known_zero): while x0 holds the zeros the library wrote, the first SpMV requests no x value on interior grid rows
(csrc/spmv_kernels.hip stencil5_rowlds_zero_kernel) and the flush of x starts from 0.0 in registers (csrc/cg_kernels.hip
cg_flush_x_kernel, x_in == nullptr); with any x0 the first launch stores r0 once, as p0, and iteration 0's r update reads it there
(cg_update_r_from_kernel). Every result must be what the launches of before compute (set_option("zero_start", 0)), bit for bit."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import cg_restatement as CG
import tile_classes as T
from conftest import ROOT
from test_distributed import free_port

ZERO_X, R0_ONCE = 1, 2  # bits of CgSlab.initial_form()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rhs(n, seed):
    """Random, with a handful of +0.0 and -0.0 entries (first and last element, both edge columns, the interior)."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n * n)
    spots = np.concatenate([[0, 1, n - 1, n, 2 * n - 1, n * n - 1, n * n - n], rng.integers(0, n * n, 40)])
    b[spots[0::2]] = 0.0
    b[spots[1::2]] = -0.0
    return b


def slab_of(B, e, n):
    B.lib().spmv_amd_reset_host_matrices()
    slab = B.CgSlab.from_matrix(B.HostMatrix(e, n * n, n * n, n))
    assert slab.coefficient_form() == 1 and slab.variant() == "stencil5/row-lds"
    return slab


def both_forms_of_the_first_launch(slab, n):
    """The initial stage with zero_start 1 and 0: forms as expected, r0, every partial and the sum equal as uint64. Returns r0."""
    slab.set_option("zero_start", 1)
    form, r0, r_vec, partials, rr = slab.initial_stage()
    assert form == ZERO_X | R0_ONCE
    assert (bits(r_vec) == 0xFFFFFFFFFFFFFFFF).all()  # r0 was stored once: the r vector was not written
    slab.set_option("zero_start", 0)
    form0, want_r0, want_r_vec, want_partials, want_rr = slab.initial_stage()
    assert form0 == 0
    assert np.array_equal(bits(want_r_vec), bits(want_r0))  # the launch of before: r and p both
    assert len(partials) == len(want_partials) == n * T.col_tiles(n)
    assert np.array_equal(bits(r0), bits(want_r0))
    assert np.array_equal(bits(partials), bits(want_partials))
    assert bits([rr])[0] == bits([want_rr])[0]
    slab.set_option("zero_start", 1)
    return r0, rr


@pytest.mark.gpu
@pytest.mark.parametrize("n", [640, 1003, 130, 129])
def test_the_first_launch_without_x_loads_equals_the_launch_of_before(Blab, O, monkeypatch, n):
    """n = 640; 1003 (odd: grid rows not 16-byte aligned, the vectors' tail element exists); 130 and 129 forced onto row-lds (a last
    column tile of two columns and of one). b random with signed zeros. zero_start 1 against 0 as uint64, and r0 against b - A 0 by
    the oracle's SpMV and axpy."""
    B = Blab
    if n < 512:
        monkeypatch.setenv("SPMV_AMD_ROWLDS_MIN_GRID", "64")
    e = O.stencil5_coo(n)
    slab = slab_of(B, e, n)
    b = rhs(n, 19 * n)
    slab.set_vectors(b=b)
    r0, rr = both_forms_of_the_first_launch(slab, n)
    rp, ci, va = O.build_csr(e, n * n)
    assert np.array_equal(bits(r0), bits(O.axpy(-1.0, O.spmv_stencil5(rp, ci, va, np.zeros(n * n), n), b)))
    assert np.isfinite(rr) and rr > 0
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["mixed", "mixed_with_an_infinite_coefficient"])
def test_the_first_launch_on_tiles_that_stream_their_coefficients(Blab, O, matrix):
    """The mixed matrix (tiles of both classes), and a copy with one interior centre set to +inf: inf x 0 = NaN comes out where the
    launch of before puts it, with the same bits (the chains still multiply every coefficient by its zero)."""
    B = Blab
    n = T.MIXED_N
    e = T.mixed_coo(O, n)
    hot = 77 * n + 300
    if matrix != "mixed":
        T.set_entry(e, hot, hot, np.inf)
    slab = slab_of(B, e, n)
    uniform, total = slab.uniform_tiles()
    assert 0 < uniform < total
    b = rhs(n, 23)
    slab.set_vectors(b=b)
    r0, rr = both_forms_of_the_first_launch(slab, n)
    if matrix == "mixed":
        rp, ci, va = O.build_csr(e, n * n)
        assert np.array_equal(bits(r0), bits(O.axpy(-1.0, O.spmv_stencil5(rp, ci, va, np.zeros(n * n), n), b)))
    else:
        assert np.array_equal(np.flatnonzero(np.isnan(r0)), [hot]) and np.isnan(rr)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


def one_solve(slab, timeline=False, **solve):
    st = slab.timeline_solve(**solve)[0] if timeline else slab.solve(**solve)
    return st.iterations, st.converged, slab.history().copy(), slab.gather()


def same(a, b):
    return a[:2] == b[:2] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3]))


def solve_with_and_without(slab, **solve):
    """(iterations, verdict, history, x) with zero_start 0, 1, 0, 1, 1: all identical to the first."""
    runs = []
    for value in (0, 1, 0, 1, 1):
        slab.set_option("zero_start", value)
        runs.append(one_solve(slab, **solve))
    slab.set_option("zero_start", 1)
    for k, r in enumerate(runs[1:]):
        assert same(r, runs[0]), (k + 1, solve)
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["4", "16"])
@pytest.mark.parametrize("matrix", ["generator_1003", "mixed"])
def test_whole_solves_are_bit_identical_with_and_without_the_zero_start(Blab, O, monkeypatch, matrix, ring):
    """x0 = 0 as the library wrote it, random right-hand side. block_rows 4 / 8, fused_direction 0 / 1 (2 on the mixed matrix, whose
    slow blocks exceed the cap), run_ahead 1 / 2: to convergence and five iterations at tol 0 under each pair; under the first, also
    detailed timers, the timeline, one iteration, and none -- where x must come back as x0."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_P_RING", ring)
    n = 1003 if matrix == "generator_1003" else T.MIXED_N
    e = O.stencil5_coo(n) if matrix == "generator_1003" else T.mixed_coo(O, n)
    slab = slab_of(B, e, n)
    slab.set_vectors(b=rhs(n, n + int(ring)))
    assert slab.initial_form() == ZERO_X | R0_ONCE
    fused = 1 if matrix == "generator_1003" else 2
    for k, (R, direction, run_ahead) in enumerate([(4, fused, 1), (8, 0, 2), (4, 0, 1), (8, fused, 2)]):
        slab.set_block_rows(R)
        slab.set_option("fused_direction", direction)
        slab.set_option("run_ahead", run_ahead)
        iterations, converged, _, _ = solve_with_and_without(slab, max_iters=80, tol=1e-10)
        assert converged == 1 and iterations > 10
        assert solve_with_and_without(slab, max_iters=5, tol=0.0)[:2] == (5, 0)
        if k == 0:
            assert solve_with_and_without(slab, max_iters=80, tol=1e-10, timers=1)[:2] == (iterations, 1)
            assert solve_with_and_without(slab, timeline=True, max_iters=80, tol=1e-10)[:2] == (iterations, 1)
            assert solve_with_and_without(slab, max_iters=1, tol=0.0)[:2] == (1, 0)
            none = solve_with_and_without(slab, max_iters=0, tol=0.0)
            assert none[0] == 0 and np.array_equal(bits(none[3]), bits(np.zeros(n * n)))
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_only_zeros_the_library_wrote_count_as_a_zero_start(Blab, O):
    """In this order on one slab: the default x0 (the zero form); an uploaded random x0 (the general form with r0 stored once; equal
    to zero_start 0 and to the restated loop); another b with x0 = None (x0 keeps its values, and the general form with them); an
    uploaded vector of zeros (never scanned: still the general form, equal to a fresh slab's zero form)."""
    B = Blab
    n, tol, max_iters = 640, 1e-8, 300
    e = O.stencil5_coo(n)
    rp, ci, va = O.build_csr(e, n * n)
    rng = np.random.default_rng(640)
    b, b2, x0 = rng.standard_normal(n * n), rng.standard_normal(n * n), 0.1 * rng.standard_normal(n * n)
    slab = slab_of(B, e, n)
    slab.set_vectors(b=b)
    assert slab.initial_form() == ZERO_X | R0_ONCE  # 1
    fresh = one_solve(slab, max_iters=max_iters, tol=tol)
    slab.set_vectors(b=b, x0=x0)  # 2
    assert slab.initial_form() == R0_ONCE
    form, r0, r_vec, _, _ = slab.initial_stage()
    assert form == R0_ONCE and (bits(r_vec) == 0xFFFFFFFFFFFFFFFF).all()
    assert np.array_equal(bits(r0), bits(O.axpy(-1.0, O.spmv_stencil5(rp, ci, va, x0, n), b)))
    got = solve_with_and_without(slab, max_iters=max_iters, tol=tol)
    wx, wh, wit, wconv = CG.solve(CG.whole_grid(O, rp, ci, va, n, "row-lds"), b, x0, max_iters, tol)
    assert got[:2] == (wit, wconv) and np.array_equal(bits(got[2]), bits(wh)) and np.array_equal(bits(got[3]), bits(wx))
    slab.set_vectors(b=b2)  # 3
    assert slab.initial_form() == R0_ONCE
    got = solve_with_and_without(slab, max_iters=5, tol=0.0)
    wx, wh, wit, wconv = CG.solve(CG.whole_grid(O, rp, ci, va, n, "row-lds"), b2, x0, 5, 0.0)  # x0 kept the values of case 2
    assert got[:2] == (wit, wconv) == (5, 0) and np.array_equal(bits(got[2]), bits(wh)) and np.array_equal(bits(got[3]), bits(wx))
    slab.set_vectors(b=b, x0=np.zeros(n * n))  # 4
    assert slab.initial_form() == R0_ONCE
    assert same(solve_with_and_without(slab, max_iters=max_iters, tol=tol), fresh)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_the_in_place_form_keeps_the_launches_of_before(Blab, O, monkeypatch):
    """SPMV_AMD_P_RING=1: outside the gate. The initial stage reports the form of before under either option -- r and p both written,
    x0 read -- and the solves are bit-identical, with the library's zeros and with uploaded ones."""
    B = Blab
    monkeypatch.setenv("SPMV_AMD_P_RING", "1")
    n = 640
    slab = slab_of(B, O.stencil5_coo(n), n)
    slab.set_vectors(b=rhs(n, 5))
    for value in (1, 0):
        slab.set_option("zero_start", value)
        assert slab.initial_form() == 0
        form, r0, r_vec, _, _ = slab.initial_stage()
        assert form == 0 and np.array_equal(bits(r0), bits(r_vec))
    ring_1 = solve_with_and_without(slab, max_iters=80, tol=1e-10)
    assert ring_1[1] == 1
    slab.set_vectors(x0=np.zeros(n * n))
    assert slab.initial_form() == 0
    assert same(solve_with_and_without(slab, max_iters=80, tol=1e-10), ring_1)
    slab.destroy()
    B.lib().spmv_amd_reset_host_matrices()


@pytest.mark.gpu
def test_a_slab_with_neighbours_keeps_the_launches_of_before():
    """Two ranks sharing the GPU over the staged communicator (tests/zero_start_worker.py), n = 512: row-lds slabs in ring mode whose
    first SpMV writes the residual, so only the gate on neighbours keeps them out. The initial stage reports the form of before
    under either option, and the solves are bit-identical."""
    world, port = 2, free_port()
    procs, logs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "zero_start_worker.py"), "512"], env=env, stdout=log,
                                      stderr=subprocess.STDOUT, text=True))
    deadline = time.monotonic() + 240
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs) or time.monotonic() > deadline:  # one failed: end the others
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.05)
    outs = []
    for p, log in zip(procs, logs):
        p.wait()
        log.seek(0)
        outs.append(log.read())
        log.close()
    assert all(p.returncode == 0 for p in procs), "\n".join(f"--- rank {r} ---\n{o[-3000:]}" for r, o in enumerate(outs))
    assert all("zero start on a slab with neighbours ok" in o for o in outs)
