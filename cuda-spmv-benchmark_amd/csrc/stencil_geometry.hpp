// stencil_geometry.hpp -- integer structure of the CSR form of an n x n 5-point
// stencil whose rows are sorted by column ([N,W,C,E,S] minus the absent ones).
// Shared by host and device code. All of it must agree bit for bit with the
// reference's index arithmetic: for interior rows
// stencil_row_start() equals calculate_interior_csr_offset()
// (reference src/spmv/spmv_stencil_csr_direct.cu:50-67).
#pragma once

#if defined(__HIPCC__)
#define SPMV_HD __host__ __device__ inline
#else
#define SPMV_HD inline
#endif

namespace spmv_amd {

// nnz in grid rows [0, i): row 0 holds 4n-2 entries, rows 1..n-2 hold 5n-2 each.
SPMV_HD long long stencil_gridrow_base(int i, int n) {
    if (i <= 0) return 0;
    long long first = 4LL * n - 2;
    if (i <= n - 1) return first + (long long)(i - 1) * (5LL * n - 2);
    return first + (long long)(n - 2) * (5LL * n - 2) + (4LL * n - 2);  // i == n: total nnz
}

// CSR start of row (i, j), valid for every row of the grid when n >= 2.
SPMV_HD long long stencil_row_start(int i, int j, int n) {
    int vertical = (i > 0) + (i < n - 1);
    long long s = stencil_gridrow_base(i, n);
    if (j > 0) s += (2 + vertical) + (long long)(j - 1) * (3 + vertical);
    return s;
}

// Same for a flat row index, also accepting row == n*n (-> nnz).
SPMV_HD long long stencil_row_start_flat(long long row, int n) {
    int i = (int)(row / n);
    int j = (int)(row - (long long)i * n);
    if (i >= n) return stencil_gridrow_base(n, n);
    return stencil_row_start(i, j, n);
}

SPMV_HD int stencil_row_nnz(int i, int j, int n) {
    return 1 + (i > 0) + (i < n - 1) + (j > 0) + (j < n - 1);
}

SPMV_HD bool stencil_is_interior(int i, int j, int n) {
    return i > 0 && i < n - 1 && j > 0 && j < n - 1;
}

// The grid 2 x 2 (x 2) aggregation makes of an axis of n points: aggregate I holds the fine points 2I and, where it exists, 2I + 1.
SPMV_HD int coarse_grid_of(int n) { return (n + 1) / 2; }

// ---- n x n x n 7-point stencil, point (k, i, j) = row k n^2 + i n + j, rows sorted by column: [D,N,W,C,E,S,U] minus the absent
// ones (D/U = -+n^2, N/S = -+n, W/E = -+1). Everything in 64 bits; n <= 674 keeps rows and nnz (7 n^3 - 6 n^2) inside int32.

// how many t' in [0, t) have a lower neighbour plus how many have an upper one, on an axis of n points (0 <= t <= n)
SPMV_HD long long stencil7_axis_neighbours(int t, int n) {
    return (long long)(t > 1 ? t - 1 : 0) + (t < n - 1 ? t : n - 1);
}

SPMV_HD long long stencil7_nnz(int n) { return 7LL * n * n * n - 6LL * n * n; }

// CSR start of row (k, i, j), valid for every row of the grid, n >= 1; (n, 0, 0) gives the total. Plane k holds
// n^2 (5 + vk) - 4 n entries, grid row (k, i) n (3 + vk + vi) - 2, row (k, i, j) 1 + vk + vi + vj (v* = neighbours on that axis):
// inside a grid row with 1 <= i, k <= n - 2 row j starts at the grid row's base + 7 j - (j > 0).
SPMV_HD long long stencil7_row_start(int k, int i, int j, int n) {
    const long long nn = (long long)n * n;
    if (k >= n) return stencil7_nnz(n);
    const int vk = (k > 0) + (k < n - 1), vi = (i > 0) + (i < n - 1);
    long long s = (long long)k * (5 * nn - 4LL * n) + nn * stencil7_axis_neighbours(k, n);
    s += (long long)i * ((long long)n * (3 + vk) - 2) + (long long)n * stencil7_axis_neighbours(i, n);
    s += (long long)j * (1 + vk + vi) + stencil7_axis_neighbours(j, n);
    return s;
}

// Same for a flat row index, also accepting row == n^3 (-> nnz).
SPMV_HD long long stencil7_row_start_flat(long long row, int n) {
    const long long nn = (long long)n * n;
    const int k = (int)(row / nn);
    const long long rest = row - (long long)k * nn;
    const int i = (int)(rest / n);
    return stencil7_row_start(k, i, (int)(rest - (long long)i * n), n);
}

SPMV_HD int stencil7_row_nnz(int k, int i, int j, int n) {
    return 1 + (k > 0) + (k < n - 1) + (i > 0) + (i < n - 1) + (j > 0) + (j < n - 1);
}

// rows and nnz of the n^3 grid fit 32-bit CSR indices: 1 <= n <= 674 (7 * 674^3 - 6 * 674^2 = 2 140 548 512; 675 does not fit)
constexpr int kStencil7MaxGrid = 674;
SPMV_HD bool stencil7_fits_int32(int n) { return n >= 1 && n <= kStencil7MaxGrid; }

// The reference's closed form, kept in 32-bit int exactly as written there.
SPMV_HD int reference_interior_csr_offset(int row, int grid_size) {
    int i = row / grid_size;
    int j = row % grid_size;
    int row0_nnz = 3 + (grid_size - 2) * 4 + 3;
    int interior_row_nnz = 4 + (grid_size - 2) * 5 + 4;
    int offset = row0_nnz + (i - 1) * interior_row_nnz;
    offset += 4 + (j - 1) * 5;
    return offset;
}

}  // namespace spmv_amd
