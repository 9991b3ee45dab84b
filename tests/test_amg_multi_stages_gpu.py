"""The two launches an AMG level adds to the batched cycle (csrc/amg_multi.hip), each on caller data through the
LAB hook spmv_amd_amg_multi_stage, bit for bit per column against tests/amg_restatement.py for every k = 1..8: aggregates of every size
around the eight lanes of a group and far beyond, rows of no, one, five and 1 100 entries, a last wave that is not full, every array
between NaN paddings that keep their bits, an inf in a row no aggregate owns, and a NaN in one column that reaches no other. (Poison in
the rows that ARE owned, in one column of the block, is tests/test_poison_csr_gpu.py's.)"""
import functools

import numpy as np
import pytest

import amg_restatement as AMG
from bitwise import same_bits, same_bits_nan_as_class

pytestmark = pytest.mark.gpu

KMAX = 8
PAD = 16                          # doubles of padding on either side
PAD_BITS = 0x7FF80000DEADBEEF     # a quiet NaN with a payload: a rewritten padding shows even if it is rewritten with a NaN
SIZES = [1, 2, 7, 8, 9, 16, 17, 64, 65, 1500]


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)
    yield


class Padded:
    """An array of any dtype on the device between NaN paddings (the payload stays 16-byte aligned); read() asserts the paddings'
    bits."""

    def __init__(self, B, values):
        values = np.ascontiguousarray(values)
        self.B, self.dtype = B, values.dtype
        raw = values.reshape(-1).view(np.uint8)
        self.nbytes = len(raw)
        body = (self.nbytes + 7) // 8
        host = np.full(2 * PAD + body, PAD_BITS, dtype=np.uint64)
        host.view(np.uint8)[8 * PAD:8 * PAD + self.nbytes] = raw
        self.host = host
        self.dev = B.DeviceVector(len(host))
        B.lib().spmv_amd_copy_to_device(self.dev.ptr, host.ctypes.data, host.nbytes)
        self.ptr = self.dev.ptr + 8 * PAD

    def read(self):
        out = np.empty_like(self.host)
        self.B.lib().spmv_amd_device_synchronize()
        self.B.lib().spmv_amd_copy_to_host(out.ctypes.data, self.dev.ptr, out.nbytes)
        keep = out.copy()
        keep.view(np.uint8)[8 * PAD:8 * PAD + self.nbytes] = self.host.view(np.uint8)[8 * PAD:8 * PAD + self.nbytes]
        assert np.array_equal(keep, self.host), "written outside the array"
        return out.view(np.uint8)[8 * PAD:8 * PAD + self.nbytes].copy().view(self.dtype)

    def free(self):
        self.dev.free()


def sizes_for(coarse_rows, rng):
    """The aggregate sizes of one launch: the last `coarse_rows` of SIZES, or all of SIZES among aggregates of 1..6 members, shuffled."""
    if coarse_rows <= len(SIZES):
        return SIZES[len(SIZES) - coarse_rows:]
    sizes = np.array(SIZES + rng.integers(1, 7, coarse_rows - len(SIZES)).tolist())
    return rng.permutation(sizes).tolist()


@functools.lru_cache(maxsize=None)
def level_for(coarse_rows):
    """A level made for the launch, with KMAX columns of z and r and the wanted coarse block; a launch on k columns takes the first k.
    `owned` rows are dealt to aggregates of the wanted sizes at random (members ascending), five more rows no aggregate owns; rows of 5
    entries, and some of 0, 1 and 1 100; columns anywhere in [0, rows + 2000): z is gathered far outside the aggregate. Row `lonely`
    (owned by nobody) holds an inf value, an inf in every column of r and the only reference to z's row `lonely_col`, which holds inf
    in every column too. Built once per size, never written."""
    from oracle import oracle as O

    rng = np.random.default_rng(coarse_rows)
    sizes = sizes_for(coarse_rows, rng)
    owned = int(sum(sizes))
    rows, cols = owned + 5, owned + 5 + 2000
    deal = rng.permutation(rows)
    free_rows, deal = np.sort(deal[:5]), deal[5:]
    agg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = np.concatenate([np.sort(deal[agg_ptr[I]:agg_ptr[I + 1]]) for I in range(coarse_rows)]).astype(np.int32)
    agg = np.full(rows, -1, dtype=np.int32)
    agg[members] = np.repeat(np.arange(coarse_rows), sizes)
    lengths = np.full(rows, 5)
    special = rng.permutation(members)[:min(9, owned)]
    lengths[special] = np.resize([0, 1, 1100], len(special))  # owned rows of 0, 1 and 1 100 entries
    lonely, lonely_col = int(free_rows[0]), cols - 1
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(cols - 1, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    va = rng.uniform(0.25, 3.0, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    Z, R = rng.standard_normal((cols, KMAX)), rng.standard_normal((rows, KMAX))
    ci[rp[lonely + 1] - 1] = lonely_col  # its last entry: no other row was offered the last column
    va[rp[lonely + 1] - 1] = np.inf
    Z[lonely_col, :] = np.inf
    R[lonely, :] = np.inf
    M, g = AMG.Csr(rp, ci, va), AMG.Aggregates(coarse_rows, agg, agg_ptr, members)
    want = np.stack([AMG.restrict(O.axpy(-1.0, O.spmv_csr(rp, ci, va, np.ascontiguousarray(Z[:, j])), np.ascontiguousarray(R[:, j])), g)
                     for j in range(KMAX)], axis=1)
    assert np.all(np.isfinite(want))
    for a in (rp, ci, va, agg_ptr, members, Z, R, want):
        a.setflags(write=False)
    return M, g, Z, R, cols, want


@pytest.mark.parametrize("k", range(1, KMAX + 1))
@pytest.mark.parametrize("coarse_rows", [1, 7, 8, 9, 513])
def test_residual_restrict_multi_stage(Blab, coarse_rows, k):
    """n_c = 1: one aggregate of 1 500 members alone in its wave; 7, 8, 9: a wave that is not full, full, and one aggregate in a second
    wave; 513: 65 waves, aggregates of 1, 2, 7, 8, 9, 16, 17, 64, 65 and 1 500 members among small ones. Column j of the coarse block
    has the bits of the single-vector restriction of column j, whatever k is."""
    M, g, Z8, R8, cols, want8 = level_for(coarse_rows)
    rows = AMG.rows_of(M)
    if coarse_rows == 513:
        assert set(SIZES) <= set(np.diff(g.agg_ptr).tolist()) and {0, 1, 5, 1100} <= set(np.diff(M.rp)[g.members].tolist())
    Z, R, want = np.ascontiguousarray(Z8[:, :k]), np.ascontiguousarray(R8[:, :k]), np.ascontiguousarray(want8[:, :k])
    arrays = [Padded(Blab, a) for a in (M.rp, M.ci, M.va, g.agg_ptr, g.members, Z, R, np.full((coarse_rows, k), np.nan))]
    d_rp, d_ci, d_va, d_ptr, d_mem, dz, dr, dc = arrays
    a = Blab.AmgStageArgs(rows=rows, cols=cols, coarse_rows=coarse_rows, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, agg_ptr=d_ptr.ptr,
                          members=d_mem.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
    assert Blab.amg_multi_stage("residual_restrict", k, a) == 0
    got = dc.read().reshape(coarse_rows, k)
    for j in range(k):
        assert same_bits(got[:, j], want[:, j]), (coarse_rows, k, j, int(np.sum(got[:, j] != want[:, j])))
    for dev, host in zip(arrays[:7], (M.rp, M.ci, M.va, g.agg_ptr, g.members, Z, R)):  # only read
        assert np.array_equal(dev.read().view(np.uint8), np.ascontiguousarray(host).reshape(-1).view(np.uint8))
    extra = []
    if k > 1:  # a NaN in one column of z and of r: that column's coarse values turn NaN, the others keep every bit
        sick = k // 2
        Zs, Rs = Z.copy(), R.copy()
        Zs[:, sick], Rs[:, sick] = np.nan, np.nan
        dzs, drs, dcs = Padded(Blab, Zs), Padded(Blab, Rs), Padded(Blab, np.full((coarse_rows, k), 0.5))
        a.z, a.r, a.coarse = dzs.ptr, drs.ptr, dcs.ptr
        assert Blab.amg_multi_stage("residual_restrict", k, a) == 0
        got = dcs.read().reshape(coarse_rows, k)
        for j in range(k):
            if j == sick:
                assert np.all(np.isnan(got[:, j])), (coarse_rows, k, j)
            else:
                assert same_bits(got[:, j], want[:, j]), (coarse_rows, k, j, "a NaN crossed into another column")
        a.z, a.r, a.coarse = dz.ptr, dr.ptr, dc.ptr
        extra = [dzs, drs, dcs]
    # an index outside its range is refused before the launch
    bad = g.members.copy()
    bad[-1] = rows
    d_bad = Padded(Blab, bad)
    a.members = d_bad.ptr
    assert Blab.amg_multi_stage("residual_restrict", k, a) != 0
    assert same_bits(dc.read(), want.reshape(-1))
    for d in arrays + extra + [d_bad]:
        d.free()


@pytest.mark.parametrize("k", range(1, KMAX + 1))
@pytest.mark.parametrize("rows", [1, 2, 3, 127, 128, 129, 4225])
def test_prolong_correct_multi_stage(Blab, O, rows, k):
    """1, 2, 3: less than one workgroup's first units; 127 .. 129: around half a workgroup of rows; 4 225: 17 workgroups, the last one
    not full. z is updated in place, per column O.axpy(2.0, e_c[agg], z)."""
    rng = np.random.default_rng(rows)
    coarse_rows = max(1, rows // 4)
    agg = rng.integers(0, coarse_rows, rows).astype(np.int32)
    Z, E = rng.standard_normal((rows, k)), rng.standard_normal((coarse_rows, k))
    d_agg, dz, de = Padded(Blab, agg), Padded(Blab, Z), Padded(Blab, E)
    a = Blab.AmgStageArgs(rows=rows, coarse_rows=coarse_rows, agg=d_agg.ptr, z=dz.ptr, coarse=de.ptr)
    assert Blab.amg_multi_stage("prolong_correct", k, a) == 0
    got = dz.read().reshape(rows, k)
    for j in range(k):
        want = O.axpy(2.0, np.ascontiguousarray(E[agg, j]), np.ascontiguousarray(Z[:, j]))
        assert same_bits(got[:, j], want), (rows, k, j)
    assert same_bits(de.read(), E.reshape(-1)) and np.array_equal(d_agg.read(), agg)
    if k > 1:  # a NaN column of e_c and z stays in its column
        sick = k - 1
        Zs, Es = Z.copy(), E.copy()
        Zs[:, sick], Es[:, sick] = np.nan, np.nan
        dzs, des = Padded(Blab, Zs), Padded(Blab, Es)
        a.z, a.coarse = dzs.ptr, des.ptr
        assert Blab.amg_multi_stage("prolong_correct", k, a) == 0
        assert same_bits_nan_as_class(dzs.read().reshape(rows, k), np.where(np.arange(k) == sick, np.nan, got))
        a.z, a.coarse = dz.ptr, de.ptr
        dzs.free(), des.free()
    bad = agg.copy()
    bad[rows // 2] = coarse_rows
    d_bad = Padded(Blab, bad)
    a.agg = d_bad.ptr
    before = dz.read()
    assert Blab.amg_multi_stage("prolong_correct", k, a) != 0
    assert same_bits(dz.read(), before)
    for d in (d_agg, dz, de, d_bad):
        d.free()
