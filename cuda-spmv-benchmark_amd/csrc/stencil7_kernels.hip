// stencil7_kernels.hip -- the n x n x n 7-point stencil in CSR form (operator "stencil7-csr"): generator and
// verifier of the complete pattern, and the two SpMV kernels.
//
// Arithmetic contract: EVERY row is the CSR loop -- sum = 0.0 ; sum = fma(v[k], x[col[k]], sum) for ascending k ; y = alpha sum --
// whichever kernel evaluates it, so oracle.spmv_csr is the bit-for-bit oracle of every row and the CSR operator's sequential
// kernels are a second witness on the GPU. A complete row is [D,N,W,C,E,S,U] (columns -n^2, -n, -1, 0, +1, +n, +n^2); the first
// term is fma(v, x, +0.0), never a bare product. -ffp-contract=off: the only fused multiply-adds are the explicit ones.
//
// Memory contract: 72 B per interior row (56 B of coefficients, 8 B x, 8 B y); N/S/D/U are re-used lines of x.
//   row-lds     the 2-D row-lds tile in three dimensions: one wave = 128 columns of one grid row (k, i fixed), the tile's 896
//               coefficients pulled with coalesced nontemporal loads into a wave-private LDS strip, W/E from an LDS copy of x;
//   row-direct  one thread per row, 256 columns of one grid row per workgroup (small grids, and the forced alternative).
// Unverified matrices never come here: the operator runs them through the CSR launcher ("stencil7/csr-loop").
// blockIdx -> tile mappings are performance choices only, never a correctness input.
#include "kernels.hpp"

#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = 4;
constexpr int kTileCols = 128;

// one row the CSR way: what every kernel here must equal
__device__ __forceinline__ double csr_row(const SlabCsr& m, const double* __restrict__ x, long long row) {
    const int k0 = m.row_ptr[row], k1 = m.row_ptr[row + 1];
    double sum = 0.0;
    for (int k = k0; k < k1; ++k) sum = fma(m.values[k], x[m.col_idx[k]], sum);
    return sum;
}

// the complete row [D,N,W,C,E,S,U] in the CSR loop's order
__device__ __forceinline__ double stencil7_interior(double vd, double xd, double vn, double xn, double vw, double xw, double vc, double xc,
                                                    double ve, double xe, double vs, double xs, double vu, double xu) {
    double sum = fma(vd, xd, 0.0);
    sum = fma(vn, xn, sum);
    sum = fma(vw, xw, sum);
    sum = fma(vc, xc, sum);
    sum = fma(ve, xe, sum);
    sum = fma(vs, xs, sum);
    return fma(vu, xu, sum);
}

// a row of column 0 ([D,N,C,E,S,U]) or column n-1 ([D,N,W,C,S,U]) of an interior grid row: six entries, the same order
__device__ __forceinline__ double stencil7_six(double v0, double x0, double v1, double x1, double v2, double x2, double v3, double x3,
                                               double v4, double x4, double v5, double x5) {
    double sum = fma(v0, x0, 0.0);
    sum = fma(v1, x1, sum);
    sum = fma(v2, x2, sum);
    sum = fma(v3, x3, sum);
    sum = fma(v4, x4, sum);
    return fma(v5, x5, sum);
}

// ---------------------------------------------------------------------------------
// row-lds. Workgroup = one wave = the tile (grid row g = k n + i, columns [j0, j0 + 128)); lane l owns columns j0 + l and
// j0 + 64 + l. Grid rows with 1 <= i, k <= n - 2 (all but ~4/n of them) take the fast path: row j of such a grid row starts at
// base + 7 j - (j > 0), so the run that starts ONE entry before the tile's first row puts row j0 + c at strip position 7 c for
// every c -- column 0 ([D,N,C,E,S,U]) at 1..6, column n-1 ([D,N,W,C,S,U]) at 0..5 of its seven slots. Fourteen coalesced
// nontemporal 8-byte loads per lane on a full tile; a short tile (the grid row's last one) loads only the 7 * (live columns)
// entries that feed a row -- base >= 1 and a following grid row exists, so no address leaves the array and nothing is clamped.
// x: the centre values by two plain loads per lane, W/E from their LDS copy (tile_west_east), N/S/D/U by plain loads (the lines
// the neighbouring grid rows and planes pull through L2 / Infinity Cache). All loads are issued before the skip flag is tested.
// Dead columns -- and the whole second half when n - j0 <= 64 -- load, add and store nothing. Face grid rows walk row_ptr.
// Partials: fma(x0, s0, 0) then fma(x1, s1, acc) per lane, one wave tree, slot = g * col_tiles + col_tile: rowlds_partials of
// tests/reduction_restatement.py on n^2 grid rows of n columns.
// ---------------------------------------------------------------------------------
template <bool kDot>
__global__ __launch_bounds__(64) void stencil7_rowlds_kernel(SlabCsr m, int n, const double* __restrict__ x, double* __restrict__ y,
                                                             double alpha, int col_tiles, int total_tiles, int run, int reverse,
                                                             double* __restrict__ dot_partials, const int* __restrict__ skip_flag) {
    __shared__ double strip[7 * kTileCols];
    __shared__ double xrow[kTileCols + 2];
    const int skip = skip_flag != nullptr ? __builtin_nontemporal_load(skip_flag) : 0;
    int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    if (reverse) tile = total_tiles - 1 - tile;  // same tiles, same partial slots, walked from the end
    const int lane = (int)threadIdx.x;
    const int g = tile / col_tiles;
    const int col_tile = tile - g * col_tiles;
    const int k = g / n, i = g - k * n;
    const int j0 = col_tile * kTileCols;
    const long long r0 = (long long)g * n + j0 + lane;  // the lane's first row
    const long long nn = (long long)n * n;
    double dot_acc = 0.0;
    if (i > 0 && i < n - 1 && k > 0 && k < n - 1) {
        const int live = n - j0 < kTileCols ? n - j0 : kTileCols;
        const double* __restrict__ vals = m.values + (stencil7_row_start(k, i, 0, n) + 7LL * j0 - 1 + lane);
        double c[14];
        if (live == kTileCols) {
#pragma unroll
            for (int q = 0; q < 14; ++q) c[q] = __builtin_nontemporal_load(vals + 64 * q);
        } else {
            const int entries = 7 * live;
#pragma unroll
            for (int q = 0; q < 14; ++q) c[q] = 64 * q + lane < entries ? __builtin_nontemporal_load(vals + 64 * q) : 0.0;
        }
        double xc[2], xw[2], xe[2], xn[2], xs[2], xd[2], xu[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + lane + 64 * h;
            xc[h] = xw[h] = xe[h] = xn[h] = xs[h] = xd[h] = xu[h] = 0.0;
            if (j < n) {
                const double* __restrict__ xl = x + (r0 + 64 * h);
                xc[h] = xl[0];
                xn[h] = xl[-n], xs[h] = xl[n];
                xd[h] = xl[-nn], xu[h] = xl[nn];
                // only the tile's two outer neighbours come from memory; the rest from the LDS copy below
                if (h == 0 && lane == 0 && j > 0) xw[0] = xl[-1];
                if (h == 1 && lane == 63 && j < n - 1) xe[1] = xl[1];
            }
        }
        if (skip != 0) return;
#pragma unroll
        for (int q = 0; q < 14; ++q) strip[64 * q + lane] = c[q];
        xrow[1 + lane] = xc[0];
        xrow[65 + lane] = xc[1];
        wave_lds_sync();
        tile_west_east(xrow, lane, j0, n, xw[0], xe[1], xw, xe);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + lane + 64 * h;
            if (j < n) {
                const double* __restrict__ v = strip + 7 * (lane + 64 * h);
                double sum;
                if (j > 0 && j < n - 1)
                    sum = stencil7_interior(v[0], xd[h], v[1], xn[h], v[2], xw[h], v[3], xc[h], v[4], xe[h], v[5], xs[h], v[6], xu[h]);
                else if (j == 0)  // [D,N,C,E,S,U] at strip positions 1..6
                    sum = stencil7_six(v[1], xd[h], v[2], xn[h], v[3], xc[h], v[4], xe[h], v[5], xs[h], v[6], xu[h]);
                else              // j == n-1: [D,N,W,C,S,U] at 0..5
                    sum = stencil7_six(v[0], xd[h], v[1], xn[h], v[2], xw[h], v[3], xc[h], v[4], xs[h], v[5], xu[h]);
                if (kDot) dot_acc = fma(xc[h], sum, dot_acc);
                __builtin_nontemporal_store(alpha * sum, y + (r0 + 64 * h));
            }
        }
    } else {
        // a grid row on a face of the cube: one row per lane and half, the CSR loop as it stands
        if (skip != 0) return;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (j0 + lane + 64 * h < n) {
                const long long r = r0 + 64 * h;
                const double sum = csr_row(m, x, r);
                if (kDot) dot_acc = fma(x[r], sum, dot_acc);
                y[r] = alpha * sum;
            }
        }
    }
    if (kDot) {
        dot_acc = wave_sum(dot_acc);
        if (lane == 0) dot_partials[tile] = dot_acc;
    }
}

// ---------------------------------------------------------------------------------
// row-direct: one thread per row, a workgroup is 256 columns of ONE grid row (no thread divides). Rows with all six neighbours
// read their seven coefficients at the computed offset with plain loads (a wave's strided loads share cache lines through the
// vector L1) and x at computed columns; every other row walks row_ptr. Partials: rowdirect_partials of
// tests/reduction_restatement.py -- fma(x, sum, 0) per thread, four wave trees combined as ((w0 + w1) + w2) + w3,
// slot = grid row * column blocks + column block.
// ---------------------------------------------------------------------------------
template <bool kDot>
__global__ __launch_bounds__(kBlock) void stencil7_rowdirect_kernel(SlabCsr m, int n, const double* __restrict__ x, double* __restrict__ y,
                                                                    double alpha, int col_blocks, int total_blocks, int reverse,
                                                                    double* __restrict__ dot_partials, const int* __restrict__ skip_flag) {
    __shared__ double wave_part[kWavesPerBlock];
    if (skip_flag != nullptr && *skip_flag != 0) return;
    const int block = reverse ? total_blocks - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int g = block / col_blocks;
    const int col_block = block - g * col_blocks;
    const int k = g / n, i = g - k * n;
    const int j = col_block * kBlock + (int)threadIdx.x;
    double dot_acc = 0.0;
    if (j < n) {
        const long long r = (long long)g * n + j;
        const long long nn = (long long)n * n;
        const double* __restrict__ xl = x + r;
        double sum;
        if (j > 0 && j < n - 1 && i > 0 && i < n - 1 && k > 0 && k < n - 1) {
            const double* __restrict__ v = m.values + (stencil7_row_start(k, i, 0, n) + 7LL * j - 1);
            const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6];
            sum = stencil7_interior(v0, xl[-nn], v1, xl[-n], v2, xl[-1], v3, xl[0], v4, xl[1], v5, xl[n], v6, xl[nn]);
        } else {
            sum = csr_row(m, x, r);
        }
        if (kDot) dot_acc = fma(xl[0], sum, dot_acc);
        y[r] = alpha * sum;
    }
    if (kDot) {
        dot_acc = wave_sum(dot_acc);
        if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = dot_acc;
        __syncthreads();
        if (threadIdx.x == 0) dot_partials[block] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
    }
}

// ---------------------------------------------------------------------------------
// Structure: generator and verifier of the complete 7-point pattern (one thread per row; set-up work)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void grid_point(long long row, int n, int* k, int* i, int* j) {
    const long long nn = (long long)n * n;
    *k = (int)(row / nn);
    const long long rest = row - (long long)*k * nn;
    *i = (int)(rest / n);
    *j = (int)(rest - (long long)*i * n);
}

__global__ __launch_bounds__(kBlock) void generate_stencil7_kernel(int n, long long rows, double center, double off, int* __restrict__ row_ptr,
                                                                   int* __restrict__ col_idx, double* __restrict__ values) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r > rows) return;
    if (r == rows) {
        row_ptr[r] = (int)stencil7_nnz(n);
        return;
    }
    int k, i, j;
    grid_point(r, n, &k, &i, &j);
    const long long nn = (long long)n * n;
    long long e = stencil7_row_start(k, i, j, n);
    row_ptr[r] = (int)e;
    if (k > 0) col_idx[e] = (int)(r - nn), values[e] = off, ++e;
    if (i > 0) col_idx[e] = (int)(r - n), values[e] = off, ++e;
    if (j > 0) col_idx[e] = (int)(r - 1), values[e] = off, ++e;
    col_idx[e] = (int)r, values[e] = center, ++e;
    if (j < n - 1) col_idx[e] = (int)(r + 1), values[e] = off, ++e;
    if (i < n - 1) col_idx[e] = (int)(r + n), values[e] = off, ++e;
    if (k < n - 1) col_idx[e] = (int)(r + nn), values[e] = off, ++e;
}

// the caller has checked n^3 == rows and the total nnz: start + row length never leaves the arrays
__global__ __launch_bounds__(kBlock) void verify_stencil7_kernel(SlabCsr m, int n, int* __restrict__ mismatch) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= m.n_local) return;
    int k, i, j;
    grid_point(r, n, &k, &i, &j);
    const long long nn = (long long)n * n;
    const long long start = stencil7_row_start(k, i, j, n);
    bool ok = m.row_ptr[r] == start && m.row_ptr[r + 1] - m.row_ptr[r] == stencil7_row_nnz(k, i, j, n);
    if (ok) {
        long long e = start;
        if (k > 0) ok = ok && m.col_idx[e++] == r - nn;
        if (i > 0) ok = ok && m.col_idx[e++] == r - n;
        if (j > 0) ok = ok && m.col_idx[e++] == r - 1;
        ok = ok && m.col_idx[e++] == r;
        if (j < n - 1) ok = ok && m.col_idx[e++] == r + 1;
        if (i < n - 1) ok = ok && m.col_idx[e++] == r + n;
        if (k < n - 1) ok = ok && m.col_idx[e++] == r + nn;
    }
    if (!ok) *mismatch = 1;  // benign race: every writer stores the same value
}

inline unsigned blocks_for(long long items) { return (unsigned)((items + kBlock - 1) / kBlock); }

}  // namespace

void launch_generate_stencil7_csr(int n, double center, double off, int* row_ptr, int* col_idx, double* values, hipStream_t stream) {
    const long long rows = (long long)n * n * n;
    hipLaunchKernelGGL(generate_stencil7_kernel, dim3(blocks_for(rows + 1)), dim3(kBlock), 0, stream, n, rows, center, off, row_ptr, col_idx,
                       values);
}

void launch_verify_stencil7_csr(const SlabCsr& m, int n, int* d_mismatch, hipStream_t stream) {
    if (m.n_local == 0) return;
    hipLaunchKernelGGL(verify_stencil7_kernel, dim3(blocks_for(m.n_local)), dim3(kBlock), 0, stream, m, n, d_mismatch);
}

// Consecutive row-lds tiles one XCD takes of every run of 8 * run: 1, the dispatch order. Swept on MI355X
// (profiles/r18_stencil7_bench.txt): 512^3 run 1 1.634 ms, 4 (= tiles per grid row) 1.674, 8 1.657, 64 1.713; 640^3 run 1 3.430 ms,
// 4 3.444, 5 (= tiles per grid row) 3.541, 10 3.582, 64 3.454. Unlike 2-D, most of the re-used x lines (D / U, a plane away) are
// out of an XCD's L2 whatever the run, and consecutive tiles on different XCDs stream in step.
int stencil7_xcd_run_rule(int n) {
    (void)n;
    return 1;
}

Stencil7Plan plan_stencil7(const SlabCsr& m, int n, bool verified, Stencil7Variant want, const Tunables& knobs) {
    Stencil7Plan p;
    p.n = n;
    Stencil7Variant v = want;
    if (!verified || n < 2) v = Stencil7Variant::CsrLoop;
    else if (v == Stencil7Variant::Auto) v = n >= knobs.stencil7_rowlds_min_grid ? Stencil7Variant::RowLds : Stencil7Variant::RowDirect;
    p.variant = v;
    if (v == Stencil7Variant::CsrLoop) {
        p.partials = csr_fused_dot_partials(m, CsrVariant::Auto);  // square matrices only: the caller's test (as for cusparse-csr)
        p.name = "stencil7/csr-loop";
        return p;
    }
    const int width = v == Stencil7Variant::RowLds ? kTileCols : kBlock;
    p.col_blocks = (n + width - 1) / width;
    p.partials = n * n * p.col_blocks;  // <= 674^2 * 6
    if (v == Stencil7Variant::RowLds) {
        p.xcd_run = knobs.rowlds_group > 0 ? knobs.rowlds_group : stencil7_xcd_run_rule(n);
        p.name = "stencil7/row-lds";
    } else {
        p.name = "stencil7/row-direct";
    }
    return p;
}

int launch_stencil7_spmv(const SlabCsr& m, const Stencil7Plan& p, const double* x, double* y, double alpha, double* d_dot_partials,
                         const int* d_skip_flag, bool reverse, hipStream_t stream) {
    const bool dot = d_dot_partials != nullptr;
    if (p.variant == Stencil7Variant::RowLds) {
        const dim3 grid((unsigned)xcd_padded_grid(p.partials, p.xcd_run));
        if (dot)
            hipLaunchKernelGGL((stencil7_rowlds_kernel<true>), grid, dim3(64), 0, stream, m, p.n, x, y, alpha, p.col_blocks, p.partials, p.xcd_run,
                               reverse ? 1 : 0, d_dot_partials, d_skip_flag);
        else
            hipLaunchKernelGGL((stencil7_rowlds_kernel<false>), grid, dim3(64), 0, stream, m, p.n, x, y, alpha, p.col_blocks, p.partials, p.xcd_run,
                               reverse ? 1 : 0, d_dot_partials, d_skip_flag);
    } else if (p.variant == Stencil7Variant::RowDirect) {
        const dim3 grid((unsigned)p.partials);
        if (dot)
            hipLaunchKernelGGL((stencil7_rowdirect_kernel<true>), grid, dim3(kBlock), 0, stream, m, p.n, x, y, alpha, p.col_blocks, p.partials,
                               reverse ? 1 : 0, d_dot_partials, d_skip_flag);
        else
            hipLaunchKernelGGL((stencil7_rowdirect_kernel<false>), grid, dim3(kBlock), 0, stream, m, p.n, x, y, alpha, p.col_blocks, p.partials,
                               reverse ? 1 : 0, d_dot_partials, d_skip_flag);
    } else {
        // unverified input: the CSR operator's kernels (no skip flag, no sweep direction: what cusparse-csr's launch has)
        launch_csr_spmv(m, x, y, alpha, CsrVariant::Auto, stream, dot && p.partials > 0 ? d_dot_partials : nullptr);
    }
    return dot ? p.partials : 0;
}

}  // namespace spmv_amd
