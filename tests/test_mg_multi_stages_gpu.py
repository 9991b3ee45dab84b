"""The batched multigrid cycle's own launches (csrc/multigrid_multi.hip) one at a time on caller data between
sentinels, through the LAB build's spmv_amd_mg_multi_stage: residual + restriction, prolongation + correction and term 0 for every
k = 1..8 on interleaved block vectors. Every column equals the oracle's single-column result bit for bit, inputs keep their bits,
nothing is written outside the outputs, and with every column marked done nothing is written at all."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import multigrid_restatement as MG
from bitwise import same_bits
from test_chebyshev_gpu import Guarded, stencil_random_values
from test_multigrid_gpu import GuardedBytes

pytestmark = pytest.mark.gpu

KMAX = 8


@pytest.fixture(autouse=True)
def _gpu(Blab):
    Blab.require_gpu()
    Blab.lib().spmv_amd_set_device(0)


@functools.lru_cache(maxsize=None)
def fine_level(n):
    """The random stencil of grid n as CSR, eight columns of z, r and e_c, and -- computed once, shared by every k -- the oracle's
    single-column results: r_c = restrict(r - A z) and z' = fma(2, prolong(e_c), z)."""
    from oracle import oracle as O

    e = stencil_random_values(n)
    A = MG.sorted_csr(sp.csr_matrix((e["value"], (e["row"], e["col"])), shape=(n * n, n * n)))
    rp, ci, va = A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    nc = (n + 1) // 2
    rng = np.random.default_rng(1000 + n)
    z, r, ec = rng.standard_normal((KMAX, n * n)), rng.standard_normal((KMAX, n * n)), rng.standard_normal((KMAX, nc * nc))
    rc = np.stack([MG.restrict(O.axpy(-1.0, O.spmv_stencil5(rp, ci, va, z[j], n), r[j]), n) for j in range(KMAX)])
    zp = np.stack([O.axpy(2.0, MG.prolong(ec[j], n), z[j]) for j in range(KMAX)])
    for a in (rp, ci, va, z, r, ec, rc, zp):
        a.setflags(write=False)
    return rp, ci, va, z, r, ec, rc, zp


def interleaved(columns, k):
    """(k, rows) -> the block's memory: element (row, j) at [row * k + j]."""
    return np.ascontiguousarray(columns[:k].T).ravel()


def column(block, k, j):
    return block.reshape(-1, k)[:, j]


class Shifted:
    """A Guarded block whose payload starts 8 bytes past a 16-byte boundary (odd k: the kernels' 8-byte path on every row)."""

    def __init__(self, B, values, shift):
        self.shift = shift
        self.inner = Guarded(B, np.concatenate([np.full(shift, 7.25), values]))
        self.ptr = self.inner.ptr + 8 * shift

    def read(self):
        got = self.inner.read()
        assert np.all(got[:self.shift] == 7.25), "written in front of the array"
        return got[self.shift:]

    def free(self):
        self.inner.free()


def done_records(Blab, k):
    rec = (Blab.PcgMultiColumn * k)()
    for j in range(k):
        rec[j].done, rec[j].converged = 1, 1
    return GuardedBytes(Blab, np.frombuffer(bytes(rec), dtype=np.uint8).copy())


@pytest.mark.parametrize("k", range(1, KMAX + 1))
@pytest.mark.parametrize("n", [9, 128, 129, 130, 257])
def test_residual_restrict_and_prolong(Blab, n, k):
    """9: a single short tile; 128: whole tiles; 129: a second tile with one live column and a lone last grid row; 130: a short second
    tile; 257: three tiles, odd rows 8-byte aligned only for odd k (and, for odd k, once more with every block vector 8 bytes off)."""
    rp, ci, va, z, r, ec, rc, zp = fine_level(n)
    nc = (n + 1) // 2
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, ci), GuardedBytes(Blab, va)
    done = done_records(Blab, k)
    for shift in ((0, 1) if (k % 2 == 1 and n == 257) else (0,)):
        hold = (lambda v: Shifted(Blab, v, shift)) if shift else (lambda v: Guarded(Blab, v))
        zb, rb, eb = interleaved(z, k), interleaved(r, k), interleaved(ec, k)
        dz, dr, dc, de = hold(zb), hold(rb), hold(np.full(nc * nc * k, np.nan)), hold(eb)
        a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr, cols=done.ptr)
        assert Blab.mg_multi_stage("residual_restrict", k, a) == 0  # every column done: nothing is written
        assert np.all(np.isnan(dc.read())), (n, k)
        a.cols = None
        assert Blab.mg_multi_stage("residual_restrict", k, a) == 0
        got = dc.read()
        for j in range(k):
            gj = column(got, k, j)
            assert same_bits(gj, rc[j]), (n, k, j, shift, int(np.sum(gj != rc[j])), np.nonzero(gj != rc[j])[0][:8])
        assert same_bits(dz.read(), zb) and same_bits(dr.read(), rb)  # only read
        assert same_bits(d_va.read(), va) and np.array_equal(d_rp.read(), rp) and np.array_equal(d_ci.read(), ci)

        a = Blab.MgMultiStageArgs(n=n, z=dz.ptr, coarse=de.ptr, cols=done.ptr)
        assert Blab.mg_multi_stage("prolong", k, a) == 0
        assert same_bits(dz.read(), zb), (n, k)  # every column done: z keeps its bits
        a.cols = None
        assert Blab.mg_multi_stage("prolong", k, a) == 0
        got = dz.read()
        for j in range(k):
            assert same_bits(column(got, k, j), zp[j]), (n, k, j, shift)
        assert same_bits(de.read(), eb)
        for g in (dz, dr, dc, de):
            g.free()
    for g in (d_rp, d_ci, d_va, done):
        g.free()


@pytest.mark.parametrize("k", range(1, KMAX + 1))
@pytest.mark.parametrize("n", [9, 129])
def test_term0(Blab, n, k):
    rows = n * n
    rng = np.random.default_rng(50 + n)
    r = rng.standard_normal((KMAX, rows))
    dinv = 1.0 / rng.uniform(1.0, 9.0, rows)
    c0 = 0.3125 + 1.0 / 3.0
    rb = interleaved(r, k)
    dr, dd, dz, dv = Guarded(Blab, rb), Guarded(Blab, np.full(rows * k, np.nan)), Guarded(Blab, np.full(rows * k, np.nan)), Guarded(Blab, dinv)
    done = done_records(Blab, k)
    a = Blab.MgMultiStageArgs(n=n, z=dz.ptr, r=dr.ptr, d=dd.ptr, dinv=dv.ptr, c0=c0, cols=done.ptr)
    assert Blab.mg_multi_stage("term0", k, a) == 0
    assert np.all(np.isnan(dd.read())) and np.all(np.isnan(dz.read())), (n, k)  # every column done: nothing is written
    a.cols = None
    assert Blab.mg_multi_stage("term0", k, a) == 0
    got_d, got_z = dd.read(), dz.read()
    for j in range(k):
        want = c0 * (dinv * r[j])  # u = dinv r ; d = c0 u ; z = d: one rounding each
        assert same_bits(column(got_d, k, j), want) and same_bits(column(got_z, k, j), want), (n, k, j)
    assert same_bits(dr.read(), rb) and same_bits(dv.read(), dinv)
    for g in (dr, dd, dz, dv, done):
        g.free()


def test_a_csr_that_is_no_stencil_is_refused(Blab, capfd):
    n = 9
    rp, ci, va, z, r, ec, rc, zp = fine_level(n)
    wrong = ci.copy()
    wrong[7] += 1
    d_rp, d_ci, d_va = GuardedBytes(Blab, rp), GuardedBytes(Blab, wrong), GuardedBytes(Blab, va)
    dz, dr, dc = Guarded(Blab, interleaved(z, 2)), Guarded(Blab, interleaved(r, 2)), Guarded(Blab, np.full(25 * 2, np.nan))
    a = Blab.MgMultiStageArgs(n=n, row_ptr=d_rp.ptr, col_idx=d_ci.ptr, values=d_va.ptr, z=dz.ptr, r=dr.ptr, coarse=dc.ptr)
    assert Blab.mg_multi_stage("residual_restrict", 2, a) != 0
    assert "not a complete 5-point stencil" in capfd.readouterr().err
    assert np.all(np.isnan(dc.read()))
    for g in (d_rp, d_ci, d_va, dz, dr, dc):
        g.free()
