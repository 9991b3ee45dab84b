"""numpy restatement of the dot partials of the multi-RHS kernels (block_partials in csrc/spmm_kernels.hip and csrc/cg_multi.hip):
one partial per workgroup and column, formed from the workgroup's 256 positions as 4 waves x 64 lanes -- each wave by the
__shfl_down tree, which for lane 0 is v[:half] + v[half:] from 32 down to 1, then ((w0 + w1) + w2) + w3. A dead position (a row or
grid column past the end) holds 0. Test infrastructure: tests/test_multi_rhs_stages_gpu.py compares the kernels' partials with
this bit for bit; tests/test_multi_rhs_host.py holds it against math.fsum."""
import numpy as np

BLOCK = 256
WAVE = 64


def flat():
    """Workgroup g holds rows 256 g .. 256 g + 255 (the vector kernels, spmm_rows_kernel)."""
    return ("flat",)


def grid(n):
    """Workgroup gi * ceil(n / 256) + c holds columns 256 c .. 256 c + 255 of grid row gi of an n x n grid (row-lds, row-direct)."""
    return ("grid", int(n))


def block_count(rows, layout):
    if layout[0] == "flat":
        return (rows + BLOCK - 1) // BLOCK
    n = layout[1]
    assert rows == n * n
    return n * ((n + BLOCK - 1) // BLOCK)


def positions(products, layout):
    """The products as (workgroups, 4 waves, 64 lanes), dead positions 0."""
    p = np.asarray(products, dtype=np.float64)
    if layout[0] == "flat":
        blocks = block_count(len(p), layout)
        out = np.zeros(blocks * BLOCK)
        out[:len(p)] = p
    else:
        n = layout[1]
        assert len(p) == n * n
        col_blocks = (n + BLOCK - 1) // BLOCK
        out = np.zeros((n, col_blocks * BLOCK))
        out[:, :n] = p.reshape(n, n)
    return out.reshape(-1, BLOCK // WAVE, WAVE)


def wave_tree(v):
    """Lane 0 of the shuffle tree over the last axis (64 lanes)."""
    half = WAVE // 2
    while half >= 1:
        v = v[..., :half] + v[..., half:2 * half]
        half //= 2
    return v[..., 0]


def block_partials_of(products, layout):
    """The per-workgroup partials of one column's per-row products, exactly as block_partials forms them."""
    w = wave_tree(positions(products, layout))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
