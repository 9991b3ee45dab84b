"""Host side of "stencil7-csr" (the n x n x n 7-point stencil) on the CPU: the operator table and its names, the Matrix Market
writer against the numpy COO through the library's own reader and COO -> CSR, the closed-form row start against row_ptr, and the
int32 refusals, which must be decided before any HIP call (this machine has no GPU)."""
import numpy as np
import pytest

import stencil7 as S7


def test_operator_table_names_and_export(B):
    L = B.lib()
    assert hasattr(L, "SPMV_STENCIL7_CSR")
    for asked in ("stencil7-csr", "stencil7"):
        op = L.get_operator(asked.encode())
        assert op and op.contents.name == b"stencil7-csr"
        assert all(bool(f) for f in (op.contents.init, op.contents.run_timed, op.contents.run_device, op.contents.free))
    assert B.Operator("stencil7").canonical_name == "stencil7-csr"
    assert L.spmv_amd_operator_variant(b"stencil7-csr") == b"uninitialised"
    for v in (b"row-lds", b"row-direct", b"csr-loop", b"auto", None):
        assert L.spmv_amd_operator_select_variant(b"stencil7-csr", v) == 0
    assert L.spmv_amd_operator_select_variant(b"stencil7-csr", b"row-generic") != 0


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_writer_reader_and_csr_equal_the_numpy_coo(B, O, fresh_host_matrices, tmp_path, n):
    path = str(tmp_path / f"s7_{n}.mtx")
    assert B.lib().write_matrix_market_stencil7(n, path.encode()) == 0
    m = B.load_matrix_market(path)
    N = n ** 3
    assert (m.c.rows, m.c.cols, m.c.nnz, m.c.grid_size) == (N, N, S7.nnz(n), n)
    want = S7.coo(n)
    for field in ("row", "col", "value"):  # the writer's entry order: C, W, E, N, S, D, U per point
        assert np.array_equal(m.entries[field], want[field]), field
    assert B.lib().spmv_amd_build_csr_struct(m.ptr) == 0
    rp, ci, va = B.host_csr_arrays()
    wrp, wci, wva = O.build_csr(want, N)
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci) and np.array_equal(va, wva)
    assert len(ci) == S7.nnz(n)
    assert O.spmv_csr(wrp, wci, wva, np.ones(N)).sum() == N + 6 * n * n


def test_writer_refuses_grids_outside_int32(B, tmp_path):
    for n in (0, -3, 675):
        assert B.lib().write_matrix_market_stencil7(n, str(tmp_path / "no.mtx").encode()) != 0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7])
def test_row_start_closed_form_is_row_ptr(B, O, n):
    N = n ** 3
    rp, _, _ = O.build_csr(S7.coo(n), N)
    f = B.lib().spmv_amd_stencil7_row_start
    assert [f(r, n) for r in range(N + 1)] == [int(v) for v in rp]
    assert f(-1, n) == -1 and f(N + 1, n) == -1


def test_row_start_at_the_int32_limit(B):
    f = B.lib().spmv_amd_stencil7_row_start
    n = 674
    total = 7 * n ** 3 - 6 * n ** 2
    assert total == 2140548512 <= 2 ** 31 - 1
    assert f(n ** 3, n) == total
    assert f(n ** 3 - 1, n) == total - 4  # the last corner: [D, N, W, C]
    assert f(1, n) == 4 and f(n, n) == 5 * n - 2  # corner row 0 has 4 entries; grid row (0, 0) holds 4 + 5 (n - 2) + 4
    # an interior grid row: row j starts at base + 7 j - (j > 0)
    base = f(n * n + n, n)
    assert [f(n * n + n + j, n) - base for j in (1, 2, 673)] == [6, 13, 7 * 673 - 1]
    assert f(0, 0) == -1
    # 675: the closed form itself is 64-bit and says why the size is refused
    assert f(675 ** 3, 675) == 7 * 675 ** 3 - 6 * 675 ** 2 > 2 ** 31 - 1


@pytest.mark.parametrize("n", [675, 0, -3])
def test_synthetic_init_refuses_bad_grids_before_any_hip_call(B, n):
    assert B.lib().spmv_amd_init_stencil7_synthetic(b"stencil7-csr", n) != 0
    assert B.lib().spmv_amd_init_stencil7_synthetic(b"cusparse-csr", n) != 0
    assert B.lib().spmv_amd_operator_variant(b"stencil7-csr") == b"uninitialised"


def test_unknown_names_have_no_3d_generator(B):
    assert B.lib().spmv_amd_init_stencil7_synthetic(b"nonsense", 8) != 0


def test_init_synthetic3d_needs_a_gpu(B):
    if B.lib().spmv_amd_device_count() >= 1:
        return  # a GPU is present: tests/test_stencil7_gpu.py runs the generator
    with pytest.raises(RuntimeError):
        B.Operator("stencil7-csr").init_synthetic3d(8)
