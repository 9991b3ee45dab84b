// stencil7_spmm.hip -- the block product of a complete 7-point level for k = 1..8 row-interleaved columns:
// stencil7_rowlds_kernel (stencil7_kernels.hip) on block vectors, for the level plans of the batched 3-D multigrid hierarchy
// (multigrid_multi.hip). The operator's own multi-RHS plan on "stencil7-csr" stays "spmm/csr".
//
// Arithmetic contract: stencil7_kernels.hip's -- EVERY row of every column is the CSR loop, sum = 0.0 ; sum = fma(v[e], x[col[e]], sum)
// for ascending e -- so column j of Y has the bits of "spmm/csr", of the single-vector kernels and of oracle.spmv_csr on column j.
// No alpha and no dot partials: the cycle passes neither. -ffp-contract=off: the only fused multiply-adds are the explicit ones.
//
// Memory contract: 56 B of coefficients per row, read ONCE for all K columns, + 16 K B of x and y: 56 + 16 K against 72 K for K
// single row-lds launches and 92 + 16 K for "spmm/csr" (which reads col_idx and row_ptr as well).
//   One one-wave workgroup = 128 columns of one grid row (k, i); lane l owns the pair of columns ja = j0 + 2 l, ja + 1: on a block
//   vector that pair is 2 K contiguous doubles, a wave's loads of one grid row one contiguous run. Grid rows with 1 <= i, k <= n - 2
//   take the fast path: the tile's 896 coefficients by fourteen coalesced nontemporal loads per lane into the wave-private LDS strip
//   (the layout of stencil7_rowlds_kernel; a short last tile loads only the live entries, so no address is clamped), then the columns
//   in chunks of at most 4: a chunk's x -- the pair, its N, S, D and U pairs, lane 0's W and lane 63's E -- is loaded, every load
//   before the first use (12 * 4 doubles per lane), W of ja and E of ja + 1 come from the adjacent lanes, and the chunk's 2 * 4 sums
//   leave with nontemporal stores. Face grid rows walk row_ptr, one row pair per lane.
// Indices: a row index times K is formed in 64 bits everywhere.
#include <stdint.h>

#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "multigrid_device.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {
namespace {

constexpr int kWave = 64;
constexpr int kTileCols = kStripCols;  // columns of one tile: lane l owns columns j0 + 2 l and j0 + 2 l + 1
constexpr int kChunk = 4;              // columns one pass holds in registers

template <int C>
__device__ __forceinline__ void store_run_once(double* __restrict__ p, const double (&v)[C]) {  // nontemporal: Y is written once
    auto two = [&](int q) {
        d2 t;
        t.x = v[q], t.y = v[q + 1];
        __builtin_nontemporal_store(t, reinterpret_cast<d2*>(p + q));
    };
    if ((((uintptr_t)p >> 3) & 1) == 0) {
#pragma unroll
        for (int q = 0; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) != 0) __builtin_nontemporal_store(v[C - 1], p + C - 1);
    } else {
        __builtin_nontemporal_store(v[0], p);
#pragma unroll
        for (int q = 1; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) == 0) __builtin_nontemporal_store(v[C - 1], p + C - 1);
    }
}

// columns C0 .. C0 + C - 1 of the lane's row pair, then the chunks behind them; at: the flat row (k, i, ja)
template <int K, int C0>
__device__ __forceinline__ void pair_chunks(const double* __restrict__ strip, const double* __restrict__ X, double* __restrict__ Y, long long at,
                                            long long nn, int n, int ja, int lane, bool has_a, bool has_b) {
    if constexpr (C0 < K) {
        constexpr int C = K - C0 < kChunk ? K - C0 : kChunk;
        double ca[C], cb[C], na[C], nb[C], sa[C], sb[C], da[C], db[C], ua[C], ub[C], west[C], east[C];
#pragma unroll
        for (int q = 0; q < C; ++q)
            ca[q] = cb[q] = na[q] = nb[q] = sa[q] = sb[q] = da[q] = db[q] = ua[q] = ub[q] = west[q] = east[q] = 0.0;
        if (has_a) {
            const double* __restrict__ xc = X + (at * K + C0);
            const long long up = (long long)n * K, plane = nn * K;
            load_run<C, false>(xc, ca);
            load_run<C, false>(xc - up, na);
            load_run<C, false>(xc + up, sa);
            load_run<C, false>(xc - plane, da);
            load_run<C, false>(xc + plane, ua);
            if (has_b) {
                load_run<C, false>(xc + K, cb);
                load_run<C, false>(xc - up + K, nb);
                load_run<C, false>(xc + up + K, sb);
                load_run<C, false>(xc - plane + K, db);
                load_run<C, false>(xc + plane + K, ub);
            }
            if (lane == 0 && ja > 0) load_run<C, false>(xc - K, west);
            if (lane == 63 && ja + 2 < n) load_run<C, false>(xc + 2 * K, east);
        }
        const double* __restrict__ v = strip + 7 * (2 * lane);
        double ya[C], yb[C];
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const double from_west = __shfl_up(cb[q], 1), from_east = __shfl_down(ca[q], 1);
            const double xw_a = lane > 0 ? from_west : west[q];
            const double xe_b = lane < 63 ? from_east : east[q];
            ya[q] = yb[q] = 0.0;
            if (has_a) ya[q] = strip_row7(v, ja, n, da[q], na[q], xw_a, ca[q], cb[q], sa[q], ua[q]);
            if (has_b) yb[q] = strip_row7(v + 7, ja + 1, n, db[q], nb[q], ca[q], cb[q], xe_b, sb[q], ub[q]);
        }
        if (has_a) store_run_once<C>(Y + (at * K + C0), ya);
        if (has_b) store_run_once<C>(Y + (at * K + C0) + K, yb);
        pair_chunks<K, C0 + C>(strip, X, Y, at, nn, n, ja, lane, has_a, has_b);
    }
}

template <int K>
__global__ __launch_bounds__(kWave) void stencil7_spmm_kernel(SlabCsr m, int n, const double* __restrict__ X, double* __restrict__ Y, int col_tiles,
                                                              int total_tiles, int run) {
    __shared__ double strip[7 * kTileCols];
    const int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    const int g = tile / col_tiles;  // the grid row k n + i
    const int j0 = (tile - g * col_tiles) * kTileCols;
    const int k = g / n, i = g - k * n;
    const int lane = (int)threadIdx.x;
    const int ja = j0 + 2 * lane;
    const bool has_a = ja < n, has_b = ja + 1 < n;
    const long long nn = (long long)n * n;
    const long long at = (long long)g * n + ja;
    if (i > 0 && i < n - 1 && k > 0 && k < n - 1) {
        const int live = n - j0 < kTileCols ? n - j0 : kTileCols;
        double c[14];
        load_strip(m.values + (stencil7_row_start(k, i, 0, n) + 7LL * j0 - 1 + lane), lane, 7 * live, c);
#pragma unroll
        for (int s = 0; s < 14; ++s) strip[64 * s + lane] = c[s];
        wave_lds_sync();
        pair_chunks<K, 0>(strip, X, Y, at, nn, n, ja, lane, has_a, has_b);
    } else {
        // a grid row on a face of the cube: the CSR loop as it stands, the lane's two rows
        for (int h = 0; h < 2; ++h) {
            if (ja + h >= n) break;
            const long long row = at + h;
            double sum[K];
#pragma unroll
            for (int q = 0; q < K; ++q) sum[q] = 0.0;
            for (int e = m.row_ptr[row]; e < m.row_ptr[row + 1]; ++e) {
                const double v = m.values[e];
                const double* __restrict__ xl = X + (long long)m.col_idx[e] * K;
#pragma unroll
                for (int q = 0; q < K; ++q) sum[q] = fma(v, xl[q], sum[q]);
            }
            store_run_once<K>(Y + row * K, sum);
        }
    }
}

}  // namespace

SpmmPlan plan_spmm_stencil7(const SlabCsr& m, int n) {
    SpmmPlan p;
    p.m = m;
    p.rows = p.cols = m.n_local;
    p.kind = SpmmKind::Stencil7Lds;
    p.name = "spmm/stencil7-row-lds";
    p.grid3 = n;
    p.col_blocks = (n + kTileCols - 1) / kTileCols;
    p.xcd_run = stencil7_xcd_run_rule(n);
    p.blocks = (long long)n * n * p.col_blocks;  // <= 674^2 * 6
    return p;
}

void launch_stencil7_spmm(const SpmmPlan& p, int k, const double* X, double* Y, hipStream_t stream) {
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((stencil7_spmm_kernel<decltype(K)::value>), dim3((unsigned)xcd_padded_grid(p.blocks, p.xcd_run)), dim3(kWave), 0, stream,
                           p.m, p.grid3, X, Y, p.col_blocks, (int)p.blocks, p.xcd_run);
    });
}

}  // namespace spmv_amd
