// multigrid3d_multi.hip -- the device side of the batched multigrid cycle on the 3-D hierarchy of "stencil7-csr" (DESIGN.md section 20;
// include/spmv_amd/api.h states the algebra): the two launches a 3-D level adds to multigrid_multi.hip's cycle, on block vectors of up
// to 8 row-interleaved columns (multi_rhs.hpp). The hierarchy, the cycle, term 0 and the step kernel are multigrid.hip's,
// multigrid_multi.hip's and pcg_multi.hip's; a level's block product is launch_spmm on the level's own plan.
//   residual_restrict3d_multi_kernel<K>  r_c[agg][j] = (((((((t000 + t001) + t010) + t011) + t100) + t101) + t110) + t111) per column
//                                        over the members that exist, t = fma(-1.0, (A z)_i, r_i): ONE launch, A z never stored, every
//                                        grid row's coefficients read once for all K columns; 56 + 17 K bytes per fine row
//   prolong_correct3d_multi_kernel<K>    z[i][j] = fma(2.0, e_c[agg(i)][j], z[i][j]), flat over rows x columns
// Per column every result has the bits of multigrid3d.hip's single-vector launch on that column alone: each row is the CSR loop --
// sum = fma(v[e], z[col[e]], sum) from +0.0 in ascending e --, the sums over an aggregate run in the order above. -ffp-contract=off:
// the only fused multiply-adds are the explicit ones. Every kernel reads the column records first and returns when no column is running
// (null records: all are); a stopped column beside running ones is computed like them.
// Indices: a row index times K is formed in 64 bits everywhere (674^3 rows x 8 columns pass int).
#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "multigrid.hpp"
#include "multigrid_device.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

namespace spmv_amd {
namespace {

constexpr int kWave = 64;
constexpr int kChunk = 4;  // columns one pass over a grid row holds in registers: 14 * 4 doubles of z and r per lane

// ---- residual + restriction in one launch, K columns ----
// The tile, the strip, the fast-path test, the row_ptr path and the XCD deal are residual_restrict3d_kernel's (multigrid3d.hip). A
// lane's fine pair (ja, ja + 1) of one grid row is 2 K contiguous doubles of a block vector. The single kernel keeps z on twelve grid
// rows and r on four in registers; times K that is out of reach, so here the GRID ROW is outermost and the column innermost: one
// accumulator per column lives through the block's four grid rows, and a grid row's z -- its own pair, the N, S, D and U pairs, lane
// 0's W and lane 63's E -- and r are loaded for a chunk of at most 4 columns as they are used, every load of the chunk before its
// first use (14 * 4 doubles per lane). The neighbour grid rows inside the block are read again through L1 / L2 in place of being held.
// The strip of the grid row is written once and read by every chunk; the next grid row's coefficients fly meanwhile.

template <int C>
struct RowRegs {
    double ca[C], cb[C];  // z at columns ja / ja + 1 of the grid row
    double na[C], nb[C], sa[C], sb[C], da[C], db[C], ua[C], ub[C];
    double ra[C], rb[C];
    double west[C], east[C];  // lane 0's W neighbour of ja, lane 63's E neighbour of ja + 1
};

// at: the flat row (k, i, ja); nn = n^2
template <int K, int C0, int C>
__device__ __forceinline__ void row_load(RowRegs<C>& t, const double* __restrict__ z, const double* __restrict__ r, long long at, long long nn,
                                         int n, int ja, int lane, bool has_a, bool has_b) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
        t.ca[q] = t.cb[q] = t.na[q] = t.nb[q] = t.sa[q] = t.sb[q] = t.da[q] = t.db[q] = t.ua[q] = t.ub[q] = 0.0;
        t.ra[q] = t.rb[q] = t.west[q] = t.east[q] = 0.0;
    }
    if (!has_a) return;
    const double* __restrict__ zc = z + (at * K + C0);
    const long long up = (long long)n * K, plane = nn * K;
    load_run<C, false>(zc, t.ca);
    load_run<C, false>(zc - up, t.na);
    load_run<C, false>(zc + up, t.sa);
    load_run<C, false>(zc - plane, t.da);
    load_run<C, false>(zc + plane, t.ua);
    load_run<C, true>(r + (at * K + C0), t.ra);
    if (has_b) {
        load_run<C, false>(zc + K, t.cb);
        load_run<C, false>(zc - up + K, t.nb);
        load_run<C, false>(zc + up + K, t.sb);
        load_run<C, false>(zc - plane + K, t.db);
        load_run<C, false>(zc + plane + K, t.ub);
        load_run<C, true>(r + (at * K + C0) + K, t.rb);
    }
    if (lane == 0 && ja > 0) load_run<C, false>(zc - K, t.west);
    if (lane == 63 && ja + 2 < n) load_run<C, false>(zc + 2 * K, t.east);
}

// columns C0 .. C0 + C - 1 of one grid row into their accumulators; first: the block's grid row (0, 0)
template <int K, int C0, int C>
__device__ __forceinline__ void row_sum(const RowRegs<C>& t, const double* __restrict__ strip, double (&acc)[K], bool first, int n, int ja,
                                        int lane, bool has_a, bool has_b) {
    const double* __restrict__ v = strip + 7 * (2 * lane);
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const double from_west = __shfl_up(t.cb[q], 1), from_east = __shfl_down(t.ca[q], 1);
        const double xw_a = lane > 0 ? from_west : t.west[q];
        const double xe_b = lane < 63 ? from_east : t.east[q];
        if (has_a) {
            const double ta = fma(-1.0, strip_row7(v, ja, n, t.da[q], t.na[q], xw_a, t.ca[q], t.cb[q], t.sa[q], t.ua[q]), t.ra[q]);
            acc[C0 + q] = first ? ta : acc[C0 + q] + ta;
            if (has_b) {
                const double tb = fma(-1.0, strip_row7(v + 7, ja + 1, n, t.db[q], t.nb[q], t.ca[q], t.cb[q], xe_b, t.sb[q], t.ub[q]), t.rb[q]);
                acc[C0 + q] = acc[C0 + q] + tb;
            }
        }
    }
}

// one grid row, every chunk of columns from C0 on, the strip already in LDS
template <int K, int C0>
__device__ __forceinline__ void row_chunks(const double* __restrict__ strip, const double* __restrict__ z, const double* __restrict__ r,
                                           double (&acc)[K], bool first, long long at, long long nn, int n, int ja, int lane, bool has_a,
                                           bool has_b) {
    if constexpr (C0 < K) {
        constexpr int C = K - C0 < kChunk ? K - C0 : kChunk;
        RowRegs<C> t;
        row_load<K, C0, C>(t, z, r, at, nn, n, ja, lane, has_a, has_b);
        row_sum<K, C0, C>(t, strip, acc, first, n, ja, lane, has_a, has_b);
        row_chunks<K, C0 + C>(strip, z, r, acc, first, at, nn, n, ja, lane, has_a, has_b);
    }
}

template <int K>
__global__ __launch_bounds__(kWave) void residual_restrict3d_multi_kernel(SlabCsr m, int n, const PcgMultiColumn* __restrict__ cols,
                                                                          const double* __restrict__ z, const double* __restrict__ r,
                                                                          double* __restrict__ rc, int nc, int col_tiles, int total_tiles,
                                                                          int run) {
    __shared__ double strip[7 * kStripCols];
    if (!any_running<K>(cols)) return;  // uniform over the launch
    const int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    const int g = tile / col_tiles;  // the coarse grid row Kc nc + I
    const int j0 = (tile - g * col_tiles) * kStripCols;
    const int Kc = g / nc, I = g - Kc * nc;
    const int lane = (int)threadIdx.x;
    const int ja = j0 + 2 * lane, jb = ja + 1;
    const int k0 = 2 * Kc, i0 = 2 * I;
    const bool has_a = ja < n, has_b = jb < n;
    const long long nn = (long long)n * n;
    const long long out = ((long long)g * nc + (ja >> 1)) * K;
    if (k0 >= 1 && k0 + 1 <= n - 2 && i0 >= 1 && i0 + 1 <= n - 2) {
        const int live = n - j0 < kStripCols ? n - j0 : kStripCols;
        const int entries = 7 * live;
        double c[14];
        load_strip(m.values + (stencil7_row_start(k0, i0, 0, n) + 7LL * j0 - 1 + lane), lane, entries, c);
        double acc[K];
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = 0.0;
        const long long at = (long long)k0 * nn + (long long)i0 * n + ja;  // (k0, i0, ja)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int s = 0; s < 14; ++s) strip[64 * s + lane] = c[s];
                wave_lds_sync();
                if (q * 2 + a < 3) {  // the next grid row's coefficients fly while this one's sums run
                    const int qn = a == 1 ? q + 1 : q, an = a == 1 ? 0 : 1;
                    load_strip(m.values + (stencil7_row_start(k0 + qn, i0 + an, 0, n) + 7LL * j0 - 1 + lane), lane, entries, c);
                }
                row_chunks<K, 0>(strip, z, r, acc, q == 0 && a == 0, at + q * nn + (long long)a * n, nn, n, ja, lane, has_a, has_b);
                wave_lds_sync();  // the next grid row's strip stores stay behind these reads
            }
        }
        if (has_a) store_run<K>(rc + out, acc);
    } else if (has_a) {
        // a grid row on a face of the cube in the block, a lone last plane or grid row: one thread per aggregate, the members that exist
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 2; ++q) {
                for (int a = 0; a < 2; ++a) {
                    if (k0 + q >= n || i0 + a >= n) continue;
                    const long long row = (long long)(k0 + q) * nn + (long long)(i0 + a) * n + ja;
                    const double ta = member_residual<K>(m, z, r, row, j);
                    acc = (q == 0 && a == 0) ? ta : acc + ta;
                    if (has_b) acc = acc + member_residual<K>(m, z, r, row + 1, j);
                }
            }
            rc[out + j] = acc;
        }
    }
}

// ---- prolongation + correction: z[i][j] = fma(2.0, e_c[agg(i)][j], z[i][j]), z in place; multigrid_multi.hip's flat walk, the
// aggregate from (k, i, j) as coarse_at3d forms it; the store is plain: the post-smoother's SpMM reads it ----
template <int K>
__global__ __launch_bounds__(kFlat) void prolong_correct3d_multi_kernel(long long rows, int n, int nc, const PcgMultiColumn* __restrict__ cols,
                                                                        const double* __restrict__ ec, double* __restrict__ z) {
    constexpr int V = FlatWalk<K>::V, U = FlatWalk<K>::P;
    if (!any_running<K>(cols)) return;
    const long long row0 = (long long)blockIdx.x * kFlat;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kFlat * i;
        const int t = f / U, col0 = (f - t * U) * V;
        const long long row = row0 + t;
        if (row >= rows) continue;
        const unsigned flat = (unsigned)row;  // < 674^3 < 2^31
        const unsigned g = flat / (unsigned)n, gj = flat - g * (unsigned)n;  // g = k n + i
        const unsigned gk = g / (unsigned)n, gi = g - gk * (unsigned)n;
        const long long coarse = ((long long)(gk >> 1) * nc + (gi >> 1)) * nc + (gj >> 1);
        double zv[V], ev[V];
        load_unit<V>(z + row * K + col0, zv);
        load_unit<V>(ec + coarse * K + col0, ev);
#pragma unroll
        for (int q = 0; q < V; ++q) zv[q] = fma(2.0, ev[q], zv[q]);
        store_unit<V>(z + row * K + col0, zv);
    }
}

}  // namespace

// ---- the launches: the batched cycle calls these, and so does the LAB build's spmv_amd_mg_multi_stage3d ----
void launch_residual_restrict3d_multi(int k, const SlabCsr& m, int n, const PcgMultiColumn* cols, const double* z, const double* r, double* rc) {
    const RestrictTiles t = restrict_tiles7(n);
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((residual_restrict3d_multi_kernel<decltype(K)::value>), dim3(t.grid()), dim3(kWave), 0, kBatchStream, m, n, cols, z, r,
                           rc, t.nc, t.col_tiles, t.tiles, t.run);
    });
}

void launch_prolong_correct3d_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z) {
    const long long rows = (long long)n * n * n;  // <= 674^3 < 2^31
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((prolong_correct3d_multi_kernel<decltype(K)::value>), dim3((unsigned)((rows + kFlat - 1) / kFlat)), dim3(kFlat), 0,
                           kBatchStream, rows, n, coarse_grid_of(n), cols, ec, z);
    });
}

}  // namespace spmv_amd

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_mg_multi_stage3d(const char* stage, int k, SpmvAmdMgMultiStageArgs* a) {
    return spmv_amd::mg_multi_stage(3, stage, k, a);  // multigrid_multi.hip: the one body of both stage hooks
}
#endif  // SPMV_AMD_LAB
