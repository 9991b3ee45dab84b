// spmm_kernels.hip -- one sparse matrix times k = 1..8 vectors (SpMM) on gfx950, for the "stencil5-csr" and "cusparse-csr"
// operators. Block vectors are row-interleaved, X[row * k + j] (multi_rhs.hpp).
//
// Arithmetic contract: that of stencil_row_device.hpp, for every column. Each column has its own accumulator and goes through
// the same fma chains (interior rows: the scalar helper, called per column), and the file is compiled with -ffp-contract=off, so
// column j of Y is, bit for bit, the single-vector product of column j
// (the CSR operator's own "csr/stream", "csr/row-scalar" and the oracle's order; "csr/adaptive" and "csr/wavefront" sum long
// rows as a tree and are not matched: the SpMM keeps the sequential, bit-reproducible form for every matrix).
//
// Memory contract: a STENCIL5 interior row costs 40 B of coefficients + 16 k B of x and y. The coefficients are read ONCE for
// all k columns -- that is the point of the SpMM.
//   row-lds     (the stencil operator's "stencil5/row-lds" variant): the shape of rowlds_tile_device.hpp's rowlds_tile. A workgroup
//               is four waves over 256 consecutive columns of one grid row; each wave streams its 64 rows' 320 coefficients
//               with fully coalesced nontemporal 8-byte loads into a wave-private LDS strip and reads them back as [N,W,C,E,S].
//               x rows are read per lane as 8k-byte runs (W / E are the neighbouring lanes' runs: cache hits), y leaves with
//               nontemporal stores. Workgroups are dealt to the XCDs in runs about one grid row long (kernels.hpp,
//               xcd_run_group).
//   row-direct  ("stencil5/row-direct"): the same index space, one thread per row, coefficients by plain loads at the
//               computed offset.
//   row-generic ("stencil5/row-generic", "(csr-loop)"): one thread per flat row, analytic interior rows where the structure
//               was verified, the CSR loop else.
//   csr         ("cusparse-csr"): one thread per row, the sequential ascending fma sum.
// Dot partials (the CG loop's p.Ap, per column): one per workgroup and column, wave trees then the four wave sums in wave
// order; the workgroup -> rows map depends on the matrix and the kind only, never on k.
#include <stdint.h>

#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 64;  // row-lds: columns per wave

template <int K, bool kVec>
__device__ __forceinline__ void load_row(const double* __restrict__ p, double (&o)[K]) {
    if constexpr (kVec && K % 2 == 0) {
#pragma unroll
        for (int i = 0; i < K / 2; ++i) {
            const d2 t = reinterpret_cast<const d2*>(p)[i];
            o[2 * i] = t.x, o[2 * i + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) o[i] = p[i];
    }
}

template <int K, bool kVec>
__device__ __forceinline__ void store_row_nt(double* __restrict__ p, const double (&v)[K]) {
    if constexpr (kVec && K % 2 == 0) {
#pragma unroll
        for (int i = 0; i < K / 2; ++i) {
            d2 t;
            t.x = v[2 * i], t.y = v[2 * i + 1];
            __builtin_nontemporal_store(t, reinterpret_cast<d2*>(p) + i);
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) __builtin_nontemporal_store(v[i], p + i);
    }
}

// One row by the CSR loop (rowlds_tile_device.hpp, row_reference with kAnalyticInterior = false): sum = 0, ascending fma; a column
// outside the readable range contributes 0 (halo kernel semantics). Columns col0 .. col0 + W - 1 of a block of K.
template <int K, int W, bool kVec>
__device__ __forceinline__ void csr_row_part(const SlabCsr& m, const double* __restrict__ X, long long row, int col0, double (&sum)[W]) {
    const int lo = -m.halo_before, hi = m.n_local + m.halo_after;
    const int k0 = m.row_ptr[row], k1 = m.row_ptr[row + 1];
#pragma unroll
    for (int j = 0; j < W; ++j) sum[j] = 0.0;
    for (int e = k0; e < k1; ++e) {
        const double v = m.values[e];
        const long long lc = (long long)m.col_idx[e] - m.row_offset;
        double xv[W];
        if (lc >= lo && lc < hi) {
            load_row<W, kVec>(X + lc * K + col0, xv);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) xv[j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) sum[j] = fma(v, xv[j], sum[j]);
    }
}

template <int K, bool kVec>
__device__ __forceinline__ void csr_row(const SlabCsr& m, const double* __restrict__ X, long long row, double (&sum)[K]) {
    csr_row_part<K, K, kVec>(m, X, row, 0, sum);
}

// Interior row, coefficients v = [N,W,C,E,S], every column.
template <int K>
__device__ __forceinline__ void interior_row(double v0, double v1, double v2, double v3, double v4, const double (&xn)[K],
                                             const double (&xw)[K], const double (&xc)[K], const double (&xe)[K],
                                             const double (&xs)[K], double (&sum)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = stencil5_interior(v1, xw[j], v2, xc[j], v3, xe[j], v0, xn[j], v4, xs[j]);
}

// One partial per column of the workgroup's rows: wave trees, then the four wave sums in wave order.
// Every thread of the workgroup must call it (it has a barrier).
template <int K>
__device__ __forceinline__ void block_partials(double (&d)[K], double* __restrict__ partials, long long count, long long blk) {
    __shared__ double s_wave[kBlock / 64][K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d[j] += __shfl_down(d[j], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) s_wave[threadIdx.x >> 6][j] = d[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int j = (int)threadIdx.x;
        partials[(long long)j * count + blk] = ((s_wave[0][j] + s_wave[1][j]) + s_wave[2][j]) + s_wave[3][j];
    }
}

template <int K>
__device__ __forceinline__ void row_dot(bool live, const double (&xc)[K], const double (&sum)[K], double (&d)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = live ? xc[j] * sum[j] : 0.0;
}

// ---- stencil, row-lds: four waves x 64 columns of one grid row; coefficients through a wave-private LDS strip ----
// Work of a wave: its 64 rows x k columns, walked FLAT: unit f = lane + 64 i (i < P) is row f / P, columns (f % P) * V ...
// + V - 1 (V = 2 where 16-byte accesses apply, else 1; P = k / V units per row). Every x / y access of one instruction is then
// one contiguous run of 64 V doubles -- a lane-per-row walk with 8k-byte rows touches k / 2 times as many cache lines per
// instruction and ran at 0.58 / 0.29 of 8 TB/s at k = 4 / 8 (profiles/r07_multi_rhs_lane_per_row.txt; flat: 0.63 / 0.56,
// profiles/r07_multi_rhs_bench.txt). The products x . (A x) go through LDS back to lane = row, so the dot
// partials are formed exactly as in a lane-per-row kernel: per column, independent of k.
template <int K, bool kDot, bool kVec>
__global__ __launch_bounds__(kBlock) void spmm_stencil5_rowlds_kernel(SlabCsr m, const double* __restrict__ X, double* __restrict__ Y,
                                                                     int col_blocks, int run, long long total,
                                                                     double* __restrict__ partials) {
    constexpr int V = (kVec && K % 2 == 0) ? 2 : 1;
    constexpr int P = K / V;
    __shared__ double strip[kBlock / 64][5 * kTile];
    __shared__ double prod[kDot ? kBlock / 64 : 1][kDot ? kTile * K : 1];
    const long long blk = xcd_run_tile<long long>(blockIdx.x, run);
    if (blk >= total) return;
    const int n = m.grid_size;
    const int gi = (int)(blk / col_blocks);
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int j0 = (int)(blk - (long long)gi * col_blocks) * kBlock + wave * kTile;
    const long long row0 = (long long)gi * n + j0;  // the tile's first row
    const bool interior_gridrow = gi > 0 && gi < n - 1;
    double* __restrict__ st = strip[wave];
    if (j0 < n && interior_gridrow) {
        // strip position 5 (j - j0) holds row j's first coefficient (row j0 = 0: [N,C,E,S] at 1..4), as in rowlds_tile
        const long long e = stencil_gridrow_base(gi, n) + 5LL * j0 - 1 - m.nnz_base + lane;
        double c[5];
        if (j0 == 0 || j0 + kTile > n - 1) {
            const long long hi = m.nnz_local - 1;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                long long idx = e + kTile * k;
                idx = idx < 0 ? 0 : (idx > hi ? hi : idx);
                c[k] = __builtin_nontemporal_load(m.values + idx);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) c[k] = __builtin_nontemporal_load(m.values + e + kTile * k);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) st[kTile * k + lane] = c[k];
        wave_lds_sync();
    }
    if (j0 < n) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int f = lane + kTile * i;
            const int t = f / P, col0 = (f - t * P) * V;
            const int j = j0 + t;
            double sum[V], xc[V];
#pragma unroll
            for (int q = 0; q < V; ++q) sum[q] = xc[q] = 0.0;
            if (j < n) {
                const long long at = (row0 + t) * K + col0;
                if (interior_gridrow) {
                    double xw[V], xe[V], xn[V], xs[V];
#pragma unroll
                    for (int q = 0; q < V; ++q) xw[q] = xe[q] = 0.0;
                    load_row<V, kVec>(X + at, xc);
                    load_row<V, kVec>(X + at - (long long)n * K, xn);
                    load_row<V, kVec>(X + at + (long long)n * K, xs);
                    if (j > 0) load_row<V, kVec>(X + at - K, xw);
                    if (j < n - 1) load_row<V, kVec>(X + at + K, xe);
                    const double* v = st + 5 * t;
                    if (j > 0 && j < n - 1) {
                        interior_row<V>(v[0], v[1], v[2], v[3], v[4], xn, xw, xc, xe, xs, sum);
                    }
                    // The two column chains (stencil5_first_column / stencil5_last_column of stencil_row_device.hpp) stay written out in this
                    // kernel: profiles/r14_stencil_helpers_isa_identity.txt, class C site 1, says why.
                    else if (j == 0) {  // [N,C,E,S] at strip positions 1..4, CSR-loop order
#pragma unroll
                        for (int q = 0; q < V; ++q) {
                            double s = fma(v[1], xn[q], 0.0);
                            s = fma(v[2], xc[q], s);
                            s = fma(v[3], xe[q], s);
                            sum[q] = fma(v[4], xs[q], s);
                        }
                    } else {  // j == n-1: [N,W,C,S], CSR-loop order
#pragma unroll
                        for (int q = 0; q < V; ++q) {
                            double s = fma(v[0], xn[q], 0.0);
                            s = fma(v[1], xw[q], s);
                            s = fma(v[2], xc[q], s);
                            sum[q] = fma(v[3], xs[q], s);
                        }
                    }
                } else {  // first / last grid row of the grid: the CSR loop
                    csr_row_part<K, V, kVec>(m, X, row0 + t, col0, sum);
                    if (kDot) load_row<V, kVec>(X + at, xc);
                }
                store_row_nt<V, kVec>(Y + at, sum);
            }
            if (kDot) {
#pragma unroll
                for (int q = 0; q < V; ++q) prod[wave][t * K + col0 + q] = j < n ? xc[q] * sum[q] : 0.0;
            }
        }
    }
    if (kDot) {
        double d[K];
        if (j0 < n) {
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < K; ++q) d[q] = prod[wave][lane * K + q];
        } else {
#pragma unroll
            for (int q = 0; q < K; ++q) d[q] = 0.0;
        }
        block_partials<K>(d, partials, total, blk);
    }
}

// ---- stencil, row-direct: 256 columns of one grid row, one thread per row, plain coefficient loads ----
template <int K, bool kDot, bool kVec>
__global__ __launch_bounds__(kBlock) void spmm_stencil5_rowdirect_kernel(SlabCsr m, const double* __restrict__ X, double* __restrict__ Y,
                                                                        int col_blocks, long long total, double* __restrict__ partials) {
    const long long blk = blockIdx.x;
    const int n = m.grid_size;
    const int gi = (int)(blk / col_blocks);
    const int j = (int)(blk - (long long)gi * col_blocks) * kBlock + (int)threadIdx.x;
    const bool live = j < n;
    const long long row = (long long)gi * n + j;
    double sum[K], xc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) sum[q] = xc[q] = 0.0;
    if (live) {
        if (j > 0 && j < n - 1 && gi > 0 && gi < n - 1) {
            const double* __restrict__ v = m.values + (stencil_gridrow_base(gi, n) + 5LL * j - 1 - m.nnz_base);
            const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4];
            const double* __restrict__ xl = X + row * K;
            double xw[K], xe[K], xn[K], xs[K];
            load_row<K, kVec>(xl, xc);
            load_row<K, kVec>(xl - K, xw);
            load_row<K, kVec>(xl + K, xe);
            load_row<K, kVec>(xl - (long long)n * K, xn);
            load_row<K, kVec>(xl + (long long)n * K, xs);
            interior_row<K>(v0, v1, v2, v3, v4, xn, xw, xc, xe, xs, sum);
        } else {
            csr_row<K, kVec>(m, X, row, sum);
            if (kDot) load_row<K, kVec>(X + row * K, xc);
        }
        store_row_nt<K, kVec>(Y + row * K, sum);
    }
    if (kDot) {
        double d[K];
        row_dot<K>(live, xc, sum, d);
        block_partials<K>(d, partials, total, blk);
    }
}

// ---- flat rows, one thread each: row-generic stencil (kAnalytic: computed interior rows) and the CSR operator ----
template <int K, bool kAnalytic, bool kDot, bool kVec>
__global__ __launch_bounds__(kBlock) void spmm_rows_kernel(SlabCsr m, const double* __restrict__ X, double* __restrict__ Y, long long total,
                                                          double* __restrict__ partials) {
    const long long blk = blockIdx.x;
    const long long row = blk * kBlock + threadIdx.x;
    const bool live = row < m.n_local;
    double sum[K], xc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) sum[q] = xc[q] = 0.0;
    if (live) {
        const int n = m.grid_size;
        bool done = false;
        if (kAnalytic) {
            const long long g = (long long)m.row_offset + row;
            const int i = (int)(g / n), jj = (int)(g - (long long)i * n);
            if (stencil_is_interior(i, jj, n)) {
                const double* __restrict__ v = m.values + (stencil_row_start(i, jj, n) - m.nnz_base);
                const double* __restrict__ xl = X + row * K;
                double xw[K], xe[K], xn[K], xs[K];
                load_row<K, kVec>(xl, xc);
                load_row<K, kVec>(xl - K, xw);
                load_row<K, kVec>(xl + K, xe);
                load_row<K, kVec>(xl - (long long)n * K, xn);
                load_row<K, kVec>(xl + (long long)n * K, xs);
                interior_row<K>(v[0], v[1], v[2], v[3], v[4], xn, xw, xc, xe, xs, sum);
                done = true;
            }
        }
        if (!done) {
            csr_row<K, kVec>(m, X, row, sum);
            if (kDot) load_row<K, kVec>(X + row * K, xc);
        }
        store_row_nt<K, kVec>(Y + row * K, sum);
    }
    if (kDot) {
        double d[K];
        row_dot<K>(live, xc, sum, d);
        block_partials<K>(d, partials, total, blk);
    }
}

template <int K, bool kDot, bool kVec>
void launch_kind(const SpmmPlan& p, const double* X, double* Y, double* partials, hipStream_t stream) {
    switch (p.kind) {
        case SpmmKind::StencilLds: {
            const dim3 grid((unsigned)xcd_padded_grid(p.blocks, p.xcd_run));
            hipLaunchKernelGGL((spmm_stencil5_rowlds_kernel<K, kDot, kVec>), grid, dim3(kBlock), 0, stream, p.m, X, Y, p.col_blocks, p.xcd_run,
                               p.blocks, partials);
            break;
        }
        case SpmmKind::StencilDirect:
            hipLaunchKernelGGL((spmm_stencil5_rowdirect_kernel<K, kDot, kVec>), dim3((unsigned)p.blocks), dim3(kBlock), 0, stream, p.m, X, Y,
                               p.col_blocks, p.blocks, partials);
            break;
        case SpmmKind::StencilGeneric:
            hipLaunchKernelGGL((spmm_rows_kernel<K, true, kDot, kVec>), dim3((unsigned)p.blocks), dim3(kBlock), 0, stream, p.m, X, Y, p.blocks,
                               partials);
            break;
        default:  // StencilCsrLoop, Csr
            hipLaunchKernelGGL((spmm_rows_kernel<K, false, kDot, kVec>), dim3((unsigned)p.blocks), dim3(kBlock), 0, stream, p.m, X, Y, p.blocks,
                               partials);
            break;
    }
}

template <int K>
void launch_k(const SpmmPlan& p, const double* X, double* Y, double* partials, hipStream_t stream) {
    const bool vec = K % 2 == 0 && (((uintptr_t)X | (uintptr_t)Y) & 15) == 0;
    if (partials != nullptr) {
        if (vec) launch_kind<K, true, true>(p, X, Y, partials, stream);
        else launch_kind<K, true, false>(p, X, Y, partials, stream);
    } else {
        if (vec) launch_kind<K, false, true>(p, X, Y, partials, stream);
        else launch_kind<K, false, false>(p, X, Y, partials, stream);
    }
}

// ---- (k, n) columns <-> interleaved rows ----
__global__ __launch_bounds__(kBlock) void interleave_kernel(int k, long long n, const double* __restrict__ src, double* __restrict__ dst,
                                                           int to_rows) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;  // index into the interleaved array
    if (i >= n * k) return;
    const long long row = i / k, j = i - row * k;
    if (to_rows) dst[i] = src[j * n + row];
    else dst[j * n + row] = src[i];
}

}  // namespace

SpmmPlan plan_spmm(const SlabCsr& m, Stencil5Variant stencil_variant, bool csr_operator, int rows, int cols) {
    SpmmPlan p;
    p.m = m;
    p.rows = rows;
    p.cols = cols;
    const int n = m.grid_size;
    if (csr_operator) {
        p.kind = SpmmKind::Csr;
        p.name = "spmm/csr";
    } else if (stencil_variant == Stencil5Variant::RowLds || stencil_variant == Stencil5Variant::RowDirect) {
        // the single-vector plan already required a verified stencil made of whole grid rows (plan_stencil5)
        p.kind = stencil_variant == Stencil5Variant::RowLds ? SpmmKind::StencilLds : SpmmKind::StencilDirect;
        p.name = stencil_variant == Stencil5Variant::RowLds ? "spmm/stencil5-row-lds" : "spmm/stencil5-row-direct";
    } else if (m.verified_stencil && n >= 2) {
        p.kind = SpmmKind::StencilGeneric;
        p.name = "spmm/stencil5-row-generic";
    } else {
        p.kind = SpmmKind::StencilCsrLoop;
        p.name = "spmm/stencil5-row-generic(csr-loop)";
    }
    if (p.kind == SpmmKind::StencilLds || p.kind == SpmmKind::StencilDirect) {
        p.col_blocks = (n + kBlock - 1) / kBlock;
        p.blocks = (long long)p.col_blocks * n;
        if (p.kind == SpmmKind::StencilLds) p.xcd_run = n >= 8000 ? xcd_run_group(n, kBlock, 1) : 1;
    } else {
        p.blocks = ((long long)m.n_local + kBlock - 1) / kBlock;
    }
    return p;
}

void launch_spmm(const SpmmPlan& p, int k, const double* X, double* Y, double* d_partials, hipStream_t stream) {
    if (p.rows == 0 || p.blocks == 0) return;
    if (p.kind == SpmmKind::Stencil7Lds) return launch_stencil7_spmm(p, k, X, Y, stream);  // no partials: the cycle passes none
    dispatch_k(k, [&](auto K) { launch_k<decltype(K)::value>(p, X, Y, d_partials, stream); });  // k outside 1..8: nothing
}

void launch_interleave(int k, size_t n, const double* src_columns, double* dst_interleaved, hipStream_t stream) {
    const long long items = (long long)n * k;
    if (items == 0) return;
    hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, k, (long long)n,
                       src_columns, dst_interleaved, 1);
}

void launch_deinterleave(int k, size_t n, const double* src_interleaved, double* dst_columns, hipStream_t stream) {
    const long long items = (long long)n * k;
    if (items == 0) return;
    hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, k, (long long)n,
                       src_interleaved, dst_columns, 0);
}

}  // namespace spmv_amd

// ---- the operand entry points (include/spmv_amd/api.h): one SpMM on caller data, block vectors to and from the device ----
using namespace spmv_amd;

namespace {
constexpr const char* kOperandTag = "multi-rhs";
bool fail(const char* what) { return batched_fail("CG-MULTI", what); }  // the tag these sentences have had since cg_multi.hip held them
}  // namespace

extern "C" int spmv_amd_spmm_device(const char* mode, int nrhs, const double* d_X, double* d_Y) {
    if (mode == nullptr || !check_rhs(kOperandTag, nrhs)) return 1;
    if (d_X == nullptr || d_Y == nullptr) return fail("null block vector"), 1;
    if ((((uintptr_t)d_X | (uintptr_t)d_Y) & 7) != 0) return fail("block vectors must be 8-byte aligned"), 1;
    SpmvOperator* op = get_operator(mode);
    if (op == nullptr) {
        fprintf(stderr, "[multi-rhs] unknown operator '%s'\n", mode);
        return 1;
    }
    MultiOperand o;
    if (!usable_operator(kOperandTag, op, &o)) return 1;
    launch_spmm(o.plan, nrhs, d_X, d_Y, nullptr, kBatchStream);
    HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" const char* spmv_amd_spmm_variant(const char* mode) {
    SpmvOperator* op = get_operator(mode);
    if (op == nullptr) return "unknown-operator";
    const MultiOperand o = multi_operand_of(op);
    if (!o.has_multi) return "none";
    return o.ready ? o.plan.name : "uninitialised";
}

namespace {
int move_block(int nrhs, size_t n, const double* src, double* dst, bool to_device) {
    if (!check_rhs(kOperandTag, nrhs)) return 1;
    if (src == nullptr || dst == nullptr) return fail("null block vector"), 1;
    if (n == 0) return 0;
    double* staging = device_try_alloc<double>(n * nrhs);
    if (staging == nullptr) return fail("no device memory for the staging copy"), 1;
    if (to_device) {
        upload(staging, src, n * nrhs);
        launch_interleave(nrhs, n, staging, dst, kBatchStream);
    } else {
        HIP_CHECK(hipStreamSynchronize(kBatchStream));
        launch_deinterleave(nrhs, n, src, staging, kBatchStream);
        HIP_CHECK(hipStreamSynchronize(kBatchStream));
        download(dst, staging, n * nrhs);
    }
    HIP_CHECK(hipStreamSynchronize(kBatchStream));
    device_release(staging);
    return 0;
}
}  // namespace

extern "C" int spmv_amd_block_to_device(int nrhs, size_t n, const double* host_columns, double* d_X) {
    return move_block(nrhs, n, host_columns, d_X, true);
}

extern "C" int spmv_amd_block_to_host(int nrhs, size_t n, const double* d_X, double* host_columns) {
    return move_block(nrhs, n, d_X, host_columns, false);
}
