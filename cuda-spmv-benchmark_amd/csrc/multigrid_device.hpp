// multigrid_device.hpp -- the device helpers of the multigrid kernels: multigrid.hip and multigrid3d.hip (one vector, 2-D and 3-D),
// multigrid_multi.hip and multigrid3d_multi.hip (block vectors of up to 8 row-interleaved columns); stencil7_spmm.hip takes the 3-D
// strip and the runs from here. Each helper exists once; a single-vector kernel calls the K = 1, q = 0 reading of a shared one. The
// restriction kernels themselves stay apart: the single ones hold all of z and r in registers, the batched ones walk the columns in
// chunks. Each kernel also keeps its own tile decode, its coefficient loads (2-D: the clamped loads of the two rows; 3-D: the walk of
// the four grid rows through the strip) and, in the flat batched prolongations, its own loop: as helpers those three changed the
// generated code (profiles/r30_multigrid_consolidation_isa_identity.txt). Unnamed namespace: every translation unit gets its own
// copies, and everything here is inlined into its kernels.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "multi_rhs.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace {

using spmv_amd::d2;
using spmv_amd::PcgMultiColumn;
using spmv_amd::SlabCsr;

constexpr int kStripCols = 128;  // fine columns of one residual-restriction tile: lane l owns aggregate column l of the tile
constexpr int kFlat = 256;       // workgroup of the flat batched kernels

// ---- the restriction tiles: one one-wave workgroup per (coarse grid row, 128 fine columns); lane l owns the fine columns ja = j0 + 2 l
// and jb = ja + 1. Tiles are dealt to the XCDs in runs (xcd_run_tile); the launchers pad the grid. What the single and the batched
// launcher of a dimension pass to their kernels: ----
struct RestrictTiles {
    int nc, col_tiles, tiles, run;
    unsigned grid() const { return (unsigned)spmv_amd::xcd_padded_grid(tiles, run); }
};
inline RestrictTiles restrict_tiles5(int n) {
    const int nc = spmv_amd::coarse_grid_of(n), col_tiles = (n + kStripCols - 1) / kStripCols;
    return RestrictTiles{nc, col_tiles, col_tiles * nc, spmv_amd::rowlds_xcd_run_rule(n)};
}
inline RestrictTiles restrict_tiles7(int n) {
    const int nc = spmv_amd::coarse_grid_of(n), col_tiles = (n + kStripCols - 1) / kStripCols;
    return RestrictTiles{nc, col_tiles, nc * nc * col_tiles, spmv_amd::stencil7_xcd_run_rule(n)};  // <= 337^2 * 6
}

// z or r at (grid row, columns ja, ja + 1), `at` the flat row of ja; has_b: column ja + 1 exists. A 16-byte pair where it is 16-byte
// aligned (an odd n leaves half the grid rows 8-byte aligned only: two 8-byte loads there).
template <bool kOnce>
__device__ __forceinline__ d2 load_pair(const double* __restrict__ v, long long at, bool has_b) {
    d2 out;
    if (has_b && (at & 1) == 0) {
        out = kOnce ? __builtin_nontemporal_load(reinterpret_cast<const d2*>(v + at)) : *reinterpret_cast<const d2*>(v + at);
    } else {
        out.x = kOnce ? __builtin_nontemporal_load(v + at) : v[at];
        out.y = 0.0;
        if (has_b) out.y = kOnce ? __builtin_nontemporal_load(v + at + 1) : v[at + 1];
    }
    return out;
}

// ---- 2-D: the two rows' coefficients through a wave-private LDS strip (the row-lds kernel's layout: row j of the tile at strip
// position 5 (j - j0), [N,W,C,E,S]; column 0 holds [N,C,E,S] at positions 1..4) ----
// The kernels load the two rows' 640 consecutive CSR values each (ten coalesced nontemporal loads per lane and row, addresses clamped at
// the array's ends, where the slots feed no row) and their z and r before this: every load of a tile comes before its first use.
__device__ __forceinline__ void store_strip5(double (*strip)[5 * kStripCols], int lane, const double (&c)[2][10]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 0; k < 10; ++k) strip[a][64 * k + lane] = c[a][k];
    spmv_amd::wave_lds_sync();
}

// the row sum at column j from the strip slots of that row (v = strip + 5 (j - j0)), through stencil5_row's chains
__device__ __forceinline__ double strip_row(const double* __restrict__ v, int j, int n, double xw, double xc, double xe, double xn, double xs) {
    using spmv_amd::stencil5_row;
    if (j > 0 && j < n - 1) return stencil5_row(j, n, v[1], xw, v[2], xc, v[3], xe, v[0], xn, v[4], xs);  // [N,W,C,E,S]
    if (j == 0) return stencil5_row(j, n, 0.0, xw, v[2], xc, v[3], xe, v[1], xn, v[4], xs);                // [N,C,E,S] at 1..4
    return stencil5_row(j, n, v[1], xw, v[2], xc, 0.0, xe, v[0], xn, v[3], xs);                            // [N,W,C,S]
}

// t = fma(-1.0, sum, r) of row (i, j), column q of K interleaved ones, for the row pairs off the fast path, with the sum stencil5-csr's
// SpMV gives for that row: grid rows 0 and n-1 walk the CSR in loop order (sum = 0 ; sum = fma(v[k], z[col[k]], sum), ascending k),
// an interior grid row (the partner of grid row 0 or n-1 in its pair) takes its chain on the row's own CSR entries ([N,W,C,E,S];
// column 0: [N,C,E,S]; column n-1: [N,W,C,S]). Row: the type the row index is formed in -- int passes a single vector (n <= 46340), a
// block vector's row * K needs 64 bits.
template <int K = 1, class Row = int>
__device__ __forceinline__ double residual_off_tile(const SlabCsr& m, const double* __restrict__ z, const double* __restrict__ r, int i, int j,
                                                    int q = 0) {
    using spmv_amd::stencil5_row;
    const int n = m.grid_size;
    const Row row = (Row)i * n + j;
    double sum;
    if (i > 0 && i < n - 1) {
        const double* __restrict__ v = m.values + m.row_ptr[row];
        const double* __restrict__ zl = z + row * K + q;
        const Row up = (Row)n * K;
        if (j > 0 && j < n - 1) sum = stencil5_row(j, n, v[1], zl[-K], v[2], zl[0], v[3], zl[K], v[0], zl[-up], v[4], zl[up]);
        else if (j == 0) sum = stencil5_row(j, n, 0.0, 0.0, v[1], zl[0], v[2], zl[K], v[0], zl[-up], v[3], zl[up]);
        else sum = stencil5_row(j, n, v[1], zl[-K], v[2], zl[0], 0.0, 0.0, v[0], zl[-up], v[3], zl[up]);
    } else {
        sum = 0.0;
        for (int e = m.row_ptr[row]; e < m.row_ptr[row + 1]; ++e) sum = fma(m.values[e], z[(long long)m.col_idx[e] * K + q], sum);
    }
    return fma(-1.0, sum, r[row * K + q]);
}

// ---- 3-D: one grid row's coefficients through ONE wave-private LDS strip (stencil7_rowlds_kernel's layout: the run starts one entry
// before the tile's first row, so column j0 + c sits at strip position 7 c) ----
// the row at column j of a grid row inside the cube from its strip slots (v = strip + 7 (j - j0)), in the CSR loop's order
__device__ __forceinline__ double strip_row7(const double* __restrict__ v, int j, int n, double xd, double xn, double xw, double xc, double xe,
                                             double xs, double xu) {
    double sum;
    if (j > 0 && j < n - 1) {  // [D,N,W,C,E,S,U]
        sum = fma(v[0], xd, 0.0);
        sum = fma(v[1], xn, sum);
        sum = fma(v[2], xw, sum);
        sum = fma(v[3], xc, sum);
        sum = fma(v[4], xe, sum);
        sum = fma(v[5], xs, sum);
        return fma(v[6], xu, sum);
    }
    if (j == 0) {  // [D,N,C,E,S,U] at 1..6
        sum = fma(v[1], xd, 0.0);
        sum = fma(v[2], xn, sum);
        sum = fma(v[3], xc, sum);
        sum = fma(v[4], xe, sum);
        sum = fma(v[5], xs, sum);
        return fma(v[6], xu, sum);
    }
    sum = fma(v[0], xd, 0.0);  // j == n-1: [D,N,W,C,S,U] at 0..5
    sum = fma(v[1], xn, sum);
    sum = fma(v[2], xw, sum);
    sum = fma(v[3], xc, sum);
    sum = fma(v[4], xs, sum);
    return fma(v[5], xu, sum);
}

// one grid row's tile of coefficients into registers: entries [0, `entries`) of the run that starts at vals
__device__ __forceinline__ void load_strip(const double* __restrict__ vals, int lane, int entries, double (&c)[14]) {
    if (entries == 7 * kStripCols) {
#pragma unroll
        for (int q = 0; q < 14; ++q) c[q] = __builtin_nontemporal_load(vals + 64 * q);
    } else {
#pragma unroll
        for (int q = 0; q < 14; ++q) c[q] = 64 * q + lane < entries ? __builtin_nontemporal_load(vals + 64 * q) : 0.0;
    }
}

// t = fma(-1.0, (A z)_row, r_row) of column q of K interleaved ones, the row as the CSR loop
template <int K = 1>
__device__ __forceinline__ double member_residual(const SlabCsr& m, const double* __restrict__ z, const double* __restrict__ r, long long row,
                                                  int q = 0) {
    double sum = 0.0;
    for (int e = m.row_ptr[row]; e < m.row_ptr[row + 1]; ++e) sum = fma(m.values[e], z[(long long)m.col_idx[e] * K + q], sum);
    return fma(-1.0, sum, r[row * K + q]);
}

// ---- e_c at the aggregate of a flat fine row ----
__device__ __forceinline__ double coarse_at(const double* __restrict__ ec, size_t flat, int n, int nc) {
    const int i = (int)(flat / (size_t)n), j = (int)(flat - (size_t)i * n);
    return ec[(size_t)(i >> 1) * nc + (j >> 1)];
}
__device__ __forceinline__ double coarse_at3d(const double* __restrict__ ec, unsigned flat, unsigned n, unsigned nc) {
    const unsigned g = flat / n, j = flat - g * n;  // g = k n + i
    const unsigned k = g / n, i = g - k * n;
    return ec[((size_t)(k >> 1) * nc + (i >> 1)) * nc + (j >> 1)];
}

// ---- block vectors ----
template <int K>
__device__ __forceinline__ bool any_running(const PcgMultiColumn* __restrict__ cols) {
    if (cols == nullptr) return true;
    bool running = false;
#pragma unroll
    for (int j = 0; j < K; ++j) running = running || cols[j].done == 0;
    return running;
}

// A run of C consecutive doubles: 16-byte accesses over the part that is 16-byte aligned (decided by the address: an odd row of an odd n
// with an odd K, or a block of odd K on an 8-byte pointer, starts 8 bytes off), 8-byte accesses at the ends.
template <int C, bool kOnce>
__device__ __forceinline__ void load_run(const double* __restrict__ p, double (&o)[C]) {
    auto one = [&](int q) { o[q] = kOnce ? __builtin_nontemporal_load(p + q) : p[q]; };
    auto two = [&](int q) {
        const d2* at = reinterpret_cast<const d2*>(p + q);
        const d2 t = kOnce ? __builtin_nontemporal_load(at) : *at;
        o[q] = t.x, o[q + 1] = t.y;
    };
    if ((((uintptr_t)p >> 3) & 1) == 0) {  // uniform over a wave for every caller here; every register index is a constant
#pragma unroll
        for (int q = 0; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) != 0) one(C - 1);
    } else {
        one(0);
#pragma unroll
        for (int q = 1; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) == 0) one(C - 1);
    }
}

template <int C>
__device__ __forceinline__ void store_run(double* __restrict__ p, const double (&v)[C]) {  // plain: the next launch reads it
    auto two = [&](int q) {
        d2 t;
        t.x = v[q], t.y = v[q + 1];
        *reinterpret_cast<d2*>(p + q) = t;
    };
    if ((((uintptr_t)p >> 3) & 1) == 0) {
#pragma unroll
        for (int q = 0; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) != 0) p[C - 1] = v[C - 1];
    } else {
        p[0] = v[0];
#pragma unroll
        for (int q = 1; q + 1 < C; q += 2) two(q);
        if constexpr ((C & 1) == 0) p[C - 1] = v[C - 1];
    }
}

// ---- the flat kernels: unit f = threadIdx.x + 256 i (i < P) of a workgroup's 256 rows is row f / P, columns (f % P) * V ... + V - 1,
// V = 2 for even K (16-byte accesses), 1 else, P = K / V -- the walk of the batched solvers' vector kernels (multi_rhs_device.hpp) ----
template <int K>
struct FlatWalk {
    static constexpr int V = K % 2 == 0 ? 2 : 1;
    static constexpr int P = K / V;
};

template <int V>
__device__ __forceinline__ void load_unit(const double* __restrict__ p, double (&o)[V]) {
    if constexpr (V == 2) {
        const d2 t = *reinterpret_cast<const d2*>(p);
        o[0] = t.x, o[1] = t.y;
    } else {
        o[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void store_unit(double* __restrict__ p, const double (&v)[V]) {
    if constexpr (V == 2) {
        d2 t;
        t.x = v[0], t.y = v[1];
        *reinterpret_cast<d2*>(p) = t;
    } else {
        p[0] = v[0];
    }
}

}  // namespace
