"""numpy restatement of every sum of the CG solvers, read from the kernels (not from their outputs). Test infrastructure:
tests/test_reduction_restatement.py holds it against math.fsum on the CPU, tests/test_reductions_gpu.py and
tests/test_cg_restated_gpu.py compare the device's sums and whole solves with it bit for bit.

A dot product is two steps. The PARTIALS, written by the kernel that touches the vectors:
  stream_partials      dot_partials_kernel, cg_init_residual_kernel, cg_update_r_kernel (csrc/cg_kernels.hip) and, two values side
                       by side, pcg_init_kernel / pcg_update_r_kernel (csrc/pcg.hip): one wave per 64 pairs
  rowdirect_partials   stencil5_rowdirect_kernel<true> (csrc/spmv_kernels.hip): 256 columns of one grid row
  rowlds_partials      rowlds_tile (row-lds and its block kernel, kMode 1; kMode 2 with a = b = r0): 128 columns of one grid row
  ell_partials         ell_block_dot (the ELLPACK operators' fused p.Ap): 256 rows
  (csr_restatement.stream_block_partials: the dot_partials tail of csr_stream_kernel, the general CSR operator's fused p.Ap:
                       per_block rows in the first lanes of 256; it lives with that kernel's row sums in tests/csr_restatement.py)
and their SUM (csrc/reduce_device.hpp):
  reduce               reduce_single_kernel / reduce_one_launch_kernel / stencil5_rowlds_edges_reduce_kernel
  reduce_pcg           pcg_reduce_kernel, per value
  reduce_multi         multi_reduce_slices_kernel + multi_reduce_step_kernel (csrc/cg_multi.hip), per column
Everything is float64; a fused multiply-add is the oracle's fma (numpy's a * b + c rounds twice). A sum that starts at +0.0 never
holds -0.0, so padding a tree or a strided walk with +0.0 changes no bit."""
import numpy as np

from multi_rhs_restatement import BLOCK, WAVE, wave_tree
from oracle import oracle as O

STAGE_BLOCKS = 256   # kReduceStageBlocks
SINGLE_MAX = 1024    # partials one workgroup sums alone (4 * kReduceBlock)
LDS_TILE_COLS = 128  # kLdsTileCols
MULTI_SLICE = 4096   # kReduceSlice of csrc/multi_rhs.hpp


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---------------------------------------------------------------- partials
def stream_count(n):
    """stream_grid(n): one wave per 64 pairs, at least one."""
    return max(1, ((n >> 1) + WAVE - 1) // WAVE)


def stream_partials(a, b):
    """The partials of sum a[i] * b[i] as the streaming kernels form them: lane i of the launch holds the pair (2i, 2i + 1) and
    evaluates fma(a0, b0, +0.0), then fma(a1, b1, acc); the odd last element is added by thread 0 of logical block 0 AFTER its
    pair; a lane without a pair holds +0.0; wave g writes slot g (`reverse` relabels the workgroups, not the slots)."""
    a, b = _f64(a), _f64(b)
    n = len(a)
    assert len(b) == n and n >= 1
    pairs, count = n >> 1, stream_count(n)
    lanes = np.zeros(count * WAVE)
    if pairs:
        acc = a[0:2 * pairs:2] * b[0:2 * pairs:2] + 0.0  # fma(a0, b0, +0.0): the product rounded once, -0.0 becomes +0.0
        lanes[:pairs] = O.fma(a[1:2 * pairs:2], b[1:2 * pairs:2], acc)
    if n & 1:
        lanes[0] = O.fma(a[n - 1:], b[n - 1:], lanes[:1])[0]
    return wave_tree(lanes.reshape(count, WAVE))


def dot_partials(x, y):
    """dot_partials_kernel"""
    return stream_partials(x, y)


def residual_partials(r):
    """cg_init_residual_kernel and cg_update_r_kernel: the partials of r.r of the r they have just written"""
    return stream_partials(r, r)


def stream_partials_two(r, z):
    """pcg_init_kernel / pcg_update_r_kernel: value 0 (r.r) at [g], value 1 (r.z) at [count + g]"""
    return np.concatenate([stream_partials(r, r), stream_partials(r, z)])


def _grid_rows(v, n, width):
    """v (whole grid rows of n columns) as (grid rows, column blocks, width), columns past n hold 0"""
    v = _f64(v)
    assert n >= 1 and len(v) % n == 0
    rows, blocks = len(v) // n, (n + width - 1) // width
    out = np.zeros((rows, blocks * width))
    out[:, :n] = v.reshape(rows, n)
    return out.reshape(rows, blocks, width)


def rowdirect_partials(x, s, n):
    """stencil5_rowdirect_kernel<true>: a workgroup is 256 columns of one grid row, a thread's term is fma(x, sum, 0); four wave
    trees combined as ((w0 + w1) + w2) + w3; slot = grid row * column blocks + column block. s = the row sums (A x, alpha = 1)."""
    term = _grid_rows(x, n, BLOCK) * _grid_rows(s, n, BLOCK) + 0.0
    w = wave_tree(term.reshape(-1, BLOCK // WAVE, WAVE))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def rowlds_partials(a, s, n):
    """rowlds_tile (one-row and block kernels; the global first and last grid row take the same form): a wave is 128 columns of one
    grid row, lane l holds columns j0 + l and j0 + 64 + l: fma(a0, s0, 0) then fma(a1, s1, acc), a column past n adds nothing;
    one wave tree; slot = grid row * column tiles + column tile. kMode 1: a = x, s = A x. kMode 2 (fused r0): a = s = r0."""
    A, S = _grid_rows(a, n, LDS_TILE_COLS), _grid_rows(s, n, LDS_TILE_COLS)
    rows, tiles = A.shape[:2]
    A, S = A.reshape(rows, tiles, 2, WAVE), S.reshape(rows, tiles, 2, WAVE)
    acc = A[:, :, 0, :] * S[:, :, 0, :] + 0.0
    acc = O.fma(A[:, :, 1, :], S[:, :, 1, :], acc).reshape(rows * tiles, WAVE)  # a dead column: fma(0, 0, acc) = acc
    return wave_tree(acc)


def ell_partials(x, s):
    """ell_block_dot<256>: thread r holds the plain product x[r] * sum (0.0 past the last row); wave trees, then the wave sums
    added in wave order; slot = workgroup."""
    x, s = _f64(x), _f64(s)
    blocks = (len(x) + BLOCK - 1) // BLOCK
    term = np.zeros(blocks * BLOCK)
    term[:len(x)] = x * s
    w = wave_tree(term.reshape(blocks, BLOCK // WAVE, WAVE))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


# ---------------------------------------------------------------- sums
def reduce_geometry(count):
    """(slice, slice workgroups): one workgroup up to 1024 partials, else slice = ceil(count / 256), ceil(count / slice) of them"""
    if count <= SINGLE_MAX:
        return count, 1
    slice_ = (count + STAGE_BLOCKS - 1) // STAGE_BLOCKS
    return slice_, (count + slice_ - 1) // slice_


def strided_sum(values):
    """Thread t of 256: elements t, t + 256, ... in ascending order, added to a +0.0 start. Returns the 256 accumulators."""
    values = _f64(values)
    steps = (len(values) + BLOCK - 1) // BLOCK
    padded = np.zeros(max(steps, 1) * BLOCK)
    padded[:len(values)] = values
    acc = np.zeros(BLOCK)
    for row in padded.reshape(-1, BLOCK):
        acc = acc + row
    return acc


def block_tree(v):
    """The 256-wide LDS tree over the last axis: s[t] += s[t + stride], stride 128 down to 1"""
    stride = BLOCK // 2
    while stride >= 1:
        v = v[..., :stride] + v[..., stride:2 * stride]
        stride //= 2
    return v[..., 0]


def workgroup_sum(values):
    return float(block_tree(strided_sum(values)))


def slice_sums(partials, slice_, blocks):
    partials = _f64(partials)
    return np.array([workgroup_sum(partials[i * slice_:min((i + 1) * slice_, len(partials))]) for i in range(blocks)])


def reduce(partials, extra=()):
    """The slice stage over `partials`, then ONE workgroup over [slice sums | extras] in the same way (with one slice: [its sum |
    extras], reduce_single_kernel)."""
    partials, extra = _f64(partials), _f64(extra)
    slice_, blocks = reduce_geometry(len(partials))
    return workgroup_sum(np.concatenate([slice_sums(partials, slice_, blocks), extra]))


def reduce_pcg(partials, count, nv):
    """pcg_reduce_kernel<nv>: value v at partials[v * count ...]. One workgroup: the slice's tree is the total (no second stage);
    more: the slice sums of a value, summed the same way."""
    partials = _f64(partials)
    slice_, blocks = reduce_geometry(count)
    totals = []
    for v in range(nv):
        mine = partials[v * count:(v + 1) * count]
        totals.append(workgroup_sum(mine) if blocks == 1 else workgroup_sum(slice_sums(mine, slice_, blocks)))
    return totals


def reduce_multi(partials):
    """One column of the batched solver: slices of 4096 partials (plain strided walk + tree), then always a second workgroup
    over the slice sums."""
    partials = _f64(partials)
    blocks = (len(partials) + MULTI_SLICE - 1) // MULTI_SLICE
    return workgroup_sum(slice_sums(partials, MULTI_SLICE, blocks))
