// stencil5_block_kernels.hip -- the block-tile kernels of a solver slab's CG loop (cg_slab_solve.hip; DESIGN.md sections 3, 4 and 9):
// the in-loop SpMV over tiles of 128 columns x 4 or 8 grid rows, its forms with the direction update inside and with b . b beside it,
// the r update that recomputes A p on the same tiles, the block map, and their launchers. A tile that is not uniform goes row by
// row through rowlds_tile (rowlds_tile_device.hpp), the one-row kernels' code; arithmetic contract: stencil_row_device.hpp.
// blockIdx -> tile mappings are performance choices only, never a correctness input.
#include "kernels.hpp"

#include <stdlib.h>

#include <type_traits>

#include "direction_device.hpp"
#include "rowlds_tile_device.hpp"
#include "skew_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {
namespace {

constexpr int kBlock = 256;

// What the block-tile kernels share. A block tile is 128 columns of block_rows consecutive local grid rows [li0, li0 + block_rows),
// evaluated by one wave, lane l on columns j0 + l and j0 + 64 + l. Block tile `block` of a launch range that starts at local grid
// row gi_lo, column tile fastest (block_map_kernel writes its byte at [block]):
struct BlockTile {
    int row_block, col_tile;  // block = row_block * col_tiles + col_tile
    int li0, j0;              // its first local grid row and first column
};
__device__ __forceinline__ BlockTile block_tile_at(int block, int col_tiles, int gi_lo, int block_rows) {
    BlockTile t;
    t.row_block = block / col_tiles;
    t.col_tile = block - t.row_block * col_tiles;
    t.li0 = gi_lo + t.row_block * block_rows;
    t.j0 = t.col_tile * kLdsTileCols;
    return t;
}

// x on the kRows + 2 grid rows li0 - 1 .. li0 + kRows of the tile: xv[r] = the lane's two columns of row li0 - 1 + r, xo[r] = the one
// value outside the tile that row li0 + r needs (lane 0: its W neighbour left of the tile; lane 63: its E neighbour right of it).
// Rows outside [row_lo, row_hi) -- the local grid rows of x that exist -- and columns past n are not requested and hold 0.0. Called
// before the block's map byte is known, so every block must stay inside; no rotation and no software pipeline: every load of the
// block is issued before the first value is used, so a wave has 6-10 KB in flight.
template <int kRows>
__device__ __forceinline__ void block_load_rows(const double* x, int n, int li0, int j0, int lane, int row_lo, int row_hi,
                                                double (&xv)[kRows + 2][2], double (&xo)[kRows]) {
#pragma unroll
    for (int r = 0; r < kRows + 2; ++r) {
        const int li = li0 - 1 + r;
        xv[r][0] = xv[r][1] = 0.0;
        if (li >= row_lo && li < row_hi) {
            const double* xr = x + ((long long)li * n + j0);
            if (j0 + lane < n) xv[r][0] = xr[lane];
            if (j0 + lane + 64 < n) xv[r][1] = xr[lane + 64];
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int li = li0 + r;
        xo[r] = 0.0;
        if (li < row_hi) {
            const double* xr = x + ((long long)li * n + j0);
            if (lane == 0 && j0 > 0) xo[r] = xr[-1];
            if (lane == 63 && j0 + kLdsTileCols < n) xo[r] = xr[kLdsTileCols];
        }
    }
}

constexpr int kRowDoubles = kLdsTileCols + 2;  // the LDS copy of one x row (tile_west_east)

// the tile's own kRows rows of x into LDS, one copy per grid row; wave_lds_sync() before block_fast_sums reads them
template <int kRows>
__device__ __forceinline__ void block_rows_to_lds(const double (&xv)[kRows + 2][2], double* lds, int lane) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        lds[r * kRowDoubles + 1 + lane] = xv[r + 1][0];
        lds[r * kRowDoubles + 65 + lane] = xv[r + 1][1];
    }
}

// THE FAST PATH of a block tile whose map byte is 1 (every tile uniform, all kRows rows present, global grid rows 1 .. n-2), on
// values the wave holds in registers (block_load_rows' layout) and the LDS copy of its own rows: per grid row, W / E from the copy
// (tile_west_east), the fma chains of rowlds_tile<1, false, true> on a uniform tile -- stencil5_row on the slab-wide quintuple --
// dot = fma(xc, sum, dot) over the lane's column `lane`, then `lane + 64`, wave_sum, and one partial of x . (A x) per 128 x 1 tile
// in the one-row kernel's slot, (li - gi_lo) * col_tiles + col_tile: the reduction's shape and every bit of the sum stay what the
// one-row kernel gives. kStoreAp: y = alpha * sum leaves with a nontemporal store; false: A x is not stored (the r update behind the
// launch recomputes it, cg_update_r_recompute_kernel) and everything else is the same code. kSelf: also one partial of x . x per
// tile, same slot of self_partials, in the form rowlds_tile's kMode 2 sums r0 . r0: fma(v, v, acc) in the same column order.
template <int kRows, bool kStoreAp, bool kSelf>
__device__ __forceinline__ void block_fast_sums(const double (&xv)[kRows + 2][2], const double (&xo)[kRows], const double* lds, int n,
                                                BlockTile t, int lane, double* y, double alpha, int gi_lo, int col_tiles,
                                                double* dot_partials, double* self_partials, const SymPlanes& sp) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int li = t.li0 + r;
        double xw[2], xe[2];
        tile_west_east(lds + r * kRowDoubles, lane, t.j0, n, xo[r], xo[r], xw, xe);
        double dot = 0.0, self = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = t.j0 + lane + 64 * h;
            if (j < n) {
                const double xc = xv[r + 1][h], xn = xv[r][h], xs = xv[r + 2][h];
                const double sum = stencil5_row(j, n, sp.w, xw[h], sp.c, xc, sp.e, xe[h], sp.n, xn, sp.s5, xs);
                dot = fma(xc, sum, dot);
                if constexpr (kSelf) self = fma(xc, xc, self);
                if constexpr (kStoreAp) __builtin_nontemporal_store(alpha * sum, y + ((long long)li * n + j));
            }
        }
        dot = wave_sum(dot);
        if constexpr (kSelf) self = wave_sum(self);
        if (lane == 0) {
            dot_partials[(li - gi_lo) * col_tiles + t.col_tile] = dot;
            if constexpr (kSelf) self_partials[(li - gi_lo) * col_tiles + t.col_tile] = self;
        }
    }
}

// A block tile that is not fast (block map byte 0: a tile that streams the planes, the grid's first or last grid row, a short last
// block): rowlds_tile once per grid row the block holds (block_rows, fewer at the range's end), with that row's own class, one
// partial per row in the one-row kernel's slot. lds: 5 * 128 + 130 doubles (rowlds_tile's strip and x row). Returns false for a
// launch enqueued past convergence (`skip`). kSelf: the row's own partial of x . x beside it; the lane's two values are read again
// (the lines the row has just pulled in) rather than handed out of rowlds_tile, which stays as it is.
template <bool kSelf = false>
__device__ __forceinline__ bool rowlds_block_slow_rows(const SlabCsr& m, const double* __restrict__ x, double* __restrict__ y, double alpha,
                                                       int gi_lo, int gi_hi, int gfirst, int col_tiles, BlockTile t, int block_rows, int lane,
                                                       int skip, double* __restrict__ lds, double* __restrict__ dot_partials,
                                                       double* __restrict__ self_partials, const SymPlanes& sp) {
    double* __restrict__ strip = lds;
    double* __restrict__ xrow = lds + 5 * kLdsTileCols;
    const ResidualOut none{nullptr, nullptr, nullptr};
    const int held = gi_hi - t.li0 < block_rows ? gi_hi - t.li0 : block_rows;
#pragma unroll 1
    for (int r = 0; r < held; ++r) {
        const int li = t.li0 + r;
        const int uniform = rowlds_tile_class(sp, li, col_tiles, t.col_tile);
        double dot = 0.0;
        if (!rowlds_tile<1, false, true>(m, x, y, alpha, li, gfirst + li, t.j0, lane, skip, strip, xrow, none, &dot, sp, uniform)) return false;
        double self = 0.0;
        if constexpr (kSelf) {
            const int n = m.grid_size;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = t.j0 + lane + 64 * h;
                if (j < n) {
                    const double v = x[(long long)li * n + j];
                    self = fma(v, v, self);
                }
            }
            self = wave_sum(self);
        }
        if (lane == 0) {
            dot_partials[(li - gi_lo) * col_tiles + t.col_tile] = dot;
            if constexpr (kSelf) self_partials[(li - gi_lo) * col_tiles + t.col_tile] = self;
        }
        wave_lds_sync();  // the next row rewrites the LDS this row's lanes have just read
    }
    return true;
}

// ---------------------------------------------------------------------------------
// The in-loop SpMV of a solver slab over BLOCK TILES. On a uniform tile the one-row kernel moves 16 B/row of unique data (x in, y
// out) but requests every x value three times (centre, north, south) from workgroups that mostly sit on different XCDs; a block
// tile reads its kRows + 2 rows of x once each, 8 (kRows + 2) / kRows + 8 B/row.
// block_map (one byte per block tile of THIS launch range, launch_block_map): 1 = the block holds kRows grid rows and every one
// of its tiles is uniform (kernels.hpp, SymPlanes) -- block_fast_sums. 0 = rowlds_block_slow_rows. Either way the partials and
// their slots are the one-row kernel's.
// kStoreAp = false (LoopShape::first_recomputed, iteration 0 on a caller's x0): the fast path does not store A p0; the other path
// stores as ever.
// ---------------------------------------------------------------------------------
template <int kRows, bool kStoreAp = true>
__global__ __launch_bounds__(64) void stencil5_rowlds_block_kernel(
    SlabCsr m, const double* __restrict__ x, double* __restrict__ y, double alpha, int gi_lo, int gi_hi, int gfirst, int col_tiles,
    int total_blocks, int run, int reverse, double* __restrict__ dot_partials, const int* __restrict__ skip_flag,
    const unsigned char* __restrict__ block_map, SymPlanes sp) {
    constexpr int kFastDoubles = kRows * kRowDoubles, kOneRowDoubles = 5 * kLdsTileCols + kRowDoubles;
    // fast path: one x row copy per grid row of the block; the other path: rowlds_tile's strip and x row
    __shared__ double lds[kFastDoubles > kOneRowDoubles ? kFastDoubles : kOneRowDoubles];
    const int skip = skip_flag != nullptr ? __builtin_nontemporal_load(skip_flag) : 0;
    const int block = rowlds_tile_of_block((int)blockIdx.x, run, total_blocks, reverse);
    if (block < 0) return;
    const BlockTile t = block_tile_at(block, col_tiles, gi_lo, kRows);
    const int lane = (int)threadIdx.x;
    const int n = m.grid_size;
    const int fast = (int)block_map[block];  // a vector load, requested in front of the x loads and tested behind them (rowlds_tile_class)
    // local grid rows of x that exist: the slab's own and the halo rows around it (SlabCsr). A fast block reads only such rows (its
    // rows are global grid rows 1 .. n-2)
    const int row_lo = -(m.halo_before / n), row_hi = (m.n_local + m.halo_after) / n;
    double xv[kRows + 2][2], xo[kRows];
    block_load_rows<kRows>(x, n, t.li0, t.j0, lane, row_lo, row_hi, xv, xo);
    if (__builtin_amdgcn_readfirstlane(fast) != 0) {
        if (skip != 0) return;
        block_rows_to_lds<kRows>(xv, lds, lane);
        wave_lds_sync();
        block_fast_sums<kRows, kStoreAp, false>(xv, xo, lds, n, t, lane, y, alpha, gi_lo, col_tiles, dot_partials, nullptr, sp);
    } else {
        rowlds_block_slow_rows(m, x, y, alpha, gi_lo, gi_hi, gfirst, col_tiles, t, kRows, lane, skip, lds, dot_partials, nullptr, sp);
    }
}

// ---------------------------------------------------------------------------------
// The direction update p' = r + beta p INSIDE the in-loop block SpMV (single-rank slabs, cg_slab.hip LoopShape::fused_direction):
// one launch instead of cg_update_p_ring_kernel followed by stencil5_rowlds_block_kernel. Between the two there is no reduction
// (beta is known before either starts), and p' was written once and read back (10.3 B/row measured) only because they were two
// launches. Here a wave reads r and p_in on its kRows + 2 rows, evaluates direction() on all of them -- the two neighbour rows are
// RE-computed, (kRows + 2) / kRows of the arithmetic, from p_in, which no wave of this launch writes (the ring's new slot is
// p_out) -- stores its own kRows rows of p' and runs block_fast_sums on the values it holds: 16 (kRows + 2) / kRows B/row read, 16
// written. Same tile -> XCD relabelling, block map, grid and partial slots as the block kernel. r and p_in are loaded together, with
// one per-lane outer load per row (below), so the loads stay this kernel's own.
// Scalars FIRST, as in cg_update_p_ring_kernel: the launch is enqueued before the host knows whether the iteration converged, and
// the launch of the converging iteration (or of one past it) reads no vector.
// A block that is not fast (map byte 0) only writes p' on the rows it holds; its A p' and partials come from
// stencil5_block_list_kernel behind this launch, which reads p' from memory.
// kStoreAp = false (LoopShape::ap_recomputed): the fast path does not store A p'; p' and the LDS copy are written as ever.
// ---------------------------------------------------------------------------------
template <int kRows, bool kStoreAp = true>
__global__ __launch_bounds__(64) void stencil5_direction_block_kernel(
    SlabCsr m, const CgScalars* __restrict__ s, int iteration, int fma_form, const double* __restrict__ rvec, const double* __restrict__ p_in,
    double* __restrict__ p_out, double* __restrict__ y, double alpha, int gi_lo, int gi_hi, int col_tiles, int total_blocks, int run, int reverse,
    double* __restrict__ dot_partials, const unsigned char* __restrict__ block_map, SymPlanes sp) {
    __shared__ double lds[kRows * kRowDoubles];  // one p' row copy per grid row of the block
    if (s->iterations != iteration || s->converged != 0) return;
    const double beta = s->beta;
    const int block = rowlds_tile_of_block((int)blockIdx.x, run, total_blocks, reverse);
    if (block < 0) return;
    const BlockTile t = block_tile_at(block, col_tiles, gi_lo, kRows);
    const int li0 = t.li0, j0 = t.j0, lane = (int)threadIdx.x;
    const int n = m.grid_size;
    const int fast = (int)block_map[block];  // a vector load, requested in front of the r / p loads and tested behind them (rowlds_tile_class)
    // r has no halo rows and this launch runs on slabs without neighbours only: rows outside [0, rows) are not requested
    const int rows = m.n_local / n;
    const bool in0 = j0 + lane < n, in1 = j0 + lane + 64 < n;
    double rv[kRows + 2][2], pv[kRows + 2][2];  // rows li0 - 1 .. li0 + kRows, the lane's two columns
    double ro[kRows], po[kRows];                // lane 0: the W neighbour left of the tile; lane 63: the E neighbour right of it
#pragma unroll
    for (int r = 0; r < kRows + 2; ++r) {
        const int li = li0 - 1 + r;
        rv[r][0] = rv[r][1] = pv[r][0] = pv[r][1] = 0.0;
        if (li >= 0 && li < rows) {
            const double* __restrict__ rr = rvec + ((long long)li * n + j0);
            const double* __restrict__ pr = p_in + ((long long)li * n + j0);
            if (in0) rv[r][0] = rr[lane], pv[r][0] = pr[lane];
            if (in1) rv[r][1] = rr[lane + 64], pv[r][1] = pr[lane + 64];
        }
    }
    // one load per vector and row from a per-lane address (lane 0: column j0 - 1, lane 63: column j0 + 128): a vector load like the
    // rest, returned in order behind them (two branches on the lane number became scalar loads, each waited for on its own)
    const bool outer = (lane == 0 && j0 > 0) || (lane == 63 && j0 + kLdsTileCols < n);
    const int outer_col = lane == 0 ? -1 : kLdsTileCols + lane - 63;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int li = li0 + r;
        ro[r] = po[r] = 0.0;
        if (li < rows && outer) {
            const long long at = (long long)li * n + j0 + outer_col;
            ro[r] = rvec[at], po[r] = p_in[at];
        }
    }
    if (__builtin_amdgcn_readfirstlane(fast) != 0) {
        // p' on every row held (columns past n keep 0: what an absent neighbour contributes), then the fast path on it; the LDS copy
        // is written beside the p' stores
#pragma unroll
        for (int r = 0; r < kRows + 2; ++r) {
            pv[r][0] = in0 ? direction(rv[r][0], beta, pv[r][0], fma_form) : 0.0;
            pv[r][1] = in1 ? direction(rv[r][1], beta, pv[r][1], fma_form) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            po[r] = outer ? direction(ro[r], beta, po[r], fma_form) : 0.0;
            double* __restrict__ out = p_out + ((long long)(li0 + r) * n + j0);
            if (in0) out[lane] = pv[r + 1][0];  // plain: the next launch's loads (and the flush) re-use these lines
            if (in1) out[lane + 64] = pv[r + 1][1];
            lds[r * kRowDoubles + 1 + lane] = pv[r + 1][0];
            lds[r * kRowDoubles + 65 + lane] = pv[r + 1][1];
        }
        wave_lds_sync();
        block_fast_sums<kRows, kStoreAp, false>(pv, po, lds, n, t, lane, y, alpha, gi_lo, col_tiles, dot_partials, nullptr, sp);
    } else {
        const int held = gi_hi - li0 < kRows ? gi_hi - li0 : kRows;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r < held) {
                double* __restrict__ out = p_out + ((long long)(li0 + r) * n + j0);
                if (in0) out[lane] = direction(rv[r + 1][0], beta, pv[r + 1][0], fma_form);
                if (in1) out[lane + 64] = direction(rv[r + 1][1], beta, pv[r + 1][1], fma_form);
            }
        }
    }
}

// A p' and its partials on the block tiles the launch above left out (`list`: the range's blocks whose map byte is 0, one workgroup
// each): the block kernel's own path for such a block, on p' in memory. Same scalar test as the launch it follows.
__global__ __launch_bounds__(64) void stencil5_block_list_kernel(SlabCsr m, const CgScalars* __restrict__ s, int iteration,
                                                                 const double* __restrict__ x, double* __restrict__ y, double alpha, int gi_lo,
                                                                 int gi_hi, int gfirst, int col_tiles, int block_rows, const int* __restrict__ list,
                                                                 double* __restrict__ dot_partials, SymPlanes sp) {
    __shared__ double lds[5 * kLdsTileCols + kLdsTileCols + 2];
    if (s->iterations != iteration || s->converged != 0) return;
    const BlockTile t = block_tile_at(list[blockIdx.x], col_tiles, gi_lo, block_rows);
    rowlds_block_slow_rows(m, x, y, alpha, gi_lo, gi_hi, gfirst, col_tiles, t, block_rows, (int)threadIdx.x, 0, lds, dot_partials, nullptr, sp);
}

// ---------------------------------------------------------------------------------
// The r update that RECOMPUTES A p' (single-rank slabs, LoopShape::ap_recomputed): r -= alpha A p' with the r.r partials,
// where the fused launch above (kStoreAp = false) has not stored A p' on its fast blocks. A p' is a pure function of p', which is in
// memory anyway: 8 B/row less written there, and here p' with its seam rows is read instead of A p'. The partials must be
// cg_update_r_kernel's, one per 128 consecutive elements of the LINEAR index, so the block tiles are cut at those boundaries
// (skew_geometry.hpp): one wave takes kRows chunks, the t-th chunk that starts in each grid row of its row block, lane l the pair
// 2 l, 2 l + 1 of each as in cg_update_r_kernel. Where the row block is fast and every chunk of the wave lies inside its grid row,
// all loads -- r and p' of the pair, p' at -n and +n, the two outer neighbours -- are issued before the scalars are looked at, W / E
// come from the neighbouring lanes, and the sum is stencil5_row on the quintuple: the very chain the fused launch ran, whose store
// was 1.0 * sum. Every other wave goes chunk by chunk and element by element (ap_at): a slow row block's A p' is read from Ap, where
// stencil5_block_list_kernel stored it; a chunk that straddles two grid rows decides per element. Same tile -> XCD relabelling as
// the fused launch, so that the seam rows are found in the L2 that read them. A launch past convergence only reads.
// kFrom = true (LoopShape::first_recomputed, iteration 0): the out-of-place instance for r0 == p0 -- `p` is the one vector that is both
// (b, or ring slot 0), `rvec` is only written: r = p0 - alpha A p0. The centre pair serves as r0 too, so r0 is not loaded a second
// time; the chain and the fma are cg_update_r_from_kernel's on (the A p0 the first launch would have stored as 1.0 * sum, p0), as
// are the odd last element and the early return. p0 has no rows outside [0, rows): `whole` keeps the -n / +n loads inside.
// ---------------------------------------------------------------------------------
// A p' at element i: read where its row block is slow, recomputed where it is fast (operands outside the grid are 0.0, and
// stencil5_row ignores W in column 0 and E in column n - 1, as in the fused launch)
__device__ __forceinline__ double ap_at(long long i, int n, int rows, int block_rows, const double* __restrict__ p, const double* __restrict__ Ap,
                                        const unsigned char* __restrict__ row_fast, const SymPlanes& sp) {
    const int li = (int)(i / n), j = (int)(i - (long long)li * n);
    if (row_fast[li / block_rows] == 0) return Ap[i];
    const double xw = j > 0 ? p[i - 1] : 0.0, xe = j < n - 1 ? p[i + 1] : 0.0;
    const double xn = li > 0 ? p[i - n] : 0.0, xs = li < rows - 1 ? p[i + n] : 0.0;
    return stencil5_row(j, n, sp.w, xw, sp.c, p[i], sp.e, xe, sp.n, xn, sp.s5, xs);
}

// two consecutive doubles: one 16-byte load where the address allows it (i +- n with an even n), else two 8-byte loads
__device__ __forceinline__ d2 load_pair(const double* __restrict__ at, bool aligned) {
    if (aligned) return *reinterpret_cast<const d2*>(at);
    d2 v;
    v.x = at[0], v.y = at[1];
    return v;
}

template <int kRows, bool kFrom = false>
__global__ __launch_bounds__(64) void cg_update_r_recompute_kernel(size_t elements, int n, int rows, const CgScalars* __restrict__ s,
                                                                   const double* __restrict__ p, const double* __restrict__ Ap,
                                                                   double* __restrict__ rvec, double* __restrict__ partials, int col_tiles,
                                                                   int total_blocks, int run, int reverse,
                                                                   const unsigned char* __restrict__ row_fast, SymPlanes sp) {
    const int block = rowlds_tile_of_block((int)blockIdx.x, run, total_blocks, reverse);
    if (block < 0) return;
    const BlockTile tile = block_tile_at(block, col_tiles, 0, kRows);  // the whole slab: the launch range starts at local grid row 0
    const int row_block = tile.row_block, t = tile.col_tile, lane = (int)threadIdx.x;
    const long long chunks = slab::chunk_count(elements);
    const size_t pairs = elements >> 1;
    const int fast = (int)row_fast[row_block];  // a vector load, requested in front of the r / p' loads and tested behind them
    slab::SkewChunk c[kRows];
    // the unguarded -n / +n loads need grid rows above and below every row of the block (a fast block never holds the grid's first
    // or last grid row; the loads are issued before the byte is known)
    bool whole = row_block * kRows >= 1 && row_block * kRows + kRows <= rows - 1;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        c[k] = slab::skew_chunk(row_block, t, k, kRows, n, rows, chunks);
        whole = whole && c[k].inside_row;
    }
    d2 rv[kRows], pc[kRows], pn[kRows], ps[kRows];
    double po[kRows];  // lane 0: the W neighbour left of the chunk; lane 63: the E neighbour right of it
    if (whole) {
        const bool aligned = (n & 1) == 0;
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const size_t pair = (size_t)c[k].chunk * 64 + lane;
            const double* __restrict__ at = p + 2 * pair;
            if constexpr (!kFrom) rv[k] = load_once(rvec, pair);
            pc[k] = *reinterpret_cast<const d2*>(at);  // plain: the rows below and above re-use these lines
            if constexpr (kFrom) rv[k] = pc[k];         // r0 is p0: the centre pair serves as both
            pn[k] = load_pair(at - n, aligned);
            ps[k] = load_pair(at + n, aligned);
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const bool outer = (lane == 0 && c[k].start_col > 0) || (lane == 63 && c[k].start_col + slab::kChunk < n);
            const long long at = c[k].chunk * slab::kChunk + (lane == 0 ? -1 : slab::kChunk + lane - 63);
            po[k] = outer ? p[at] : 0.0;
        }
    }
    const int converged = s->converged;
    const double rr_old = s->rr_old, pAp = s->pAp;
    if (converged) return;
    const double alpha = rr_old / pAp;
    if (whole && __builtin_amdgcn_readfirstlane(fast) != 0) {
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const double from_west = __shfl_up(pc[k].y, 1), from_east = __shfl_down(pc[k].x, 1);
            const double xw = lane > 0 ? from_west : po[k], xe = lane < 63 ? from_east : po[k];
            const int j = c[k].start_col + 2 * lane;
            const double sum_x = stencil5_row(j, n, sp.w, xw, sp.c, pc[k].x, sp.e, pc[k].y, sp.n, pn[k].x, sp.s5, ps[k].x);
            const double sum_y = stencil5_row(j + 1, n, sp.w, pc[k].x, sp.c, pc[k].y, sp.e, xe, sp.n, pn[k].y, sp.s5, ps[k].y);
            d2 v = rv[k];
            v.x = fma(-alpha, sum_x, v.x);
            v.y = fma(-alpha, sum_y, v.y);
            store_once(rvec, (size_t)c[k].chunk * 64 + lane, v);
            double acc = fma(v.x, v.x, 0.0);
            acc = fma(v.y, v.y, acc);
            acc = wave_sum(acc);
            if (lane == 0) partials[c[k].chunk] = acc;
        }
        return;
    }
#pragma unroll 1
    for (int k = 0; k < kRows; ++k) {
        const slab::SkewChunk ck = slab::skew_chunk(row_block, t, k, kRows, n, rows, chunks);
        if (!ck.exists) continue;
        const size_t pair = (size_t)ck.chunk * 64 + lane;
        double acc = 0.0;
        if (pair < pairs) {
            const long long i = 2 * (long long)pair;
            d2 v;
            if constexpr (kFrom) v = *reinterpret_cast<const d2*>(p + i);
            else v = load_once(rvec, pair);
            v.x = fma(-alpha, ap_at(i, n, rows, kRows, p, Ap, row_fast, sp), v.x);
            v.y = fma(-alpha, ap_at(i + 1, n, rows, kRows, p, Ap, row_fast, sp), v.y);
            store_once(rvec, pair, v);
            acc = fma(v.x, v.x, acc);
            acc = fma(v.y, v.y, acc);
        }
        if ((elements & 1) && ck.chunk == 0 && lane == 0) {  // the odd last element, where cg_update_r_kernel adds it
            const double rl = fma(-alpha, ap_at((long long)elements - 1, n, rows, kRows, p, Ap, row_fast, sp), (kFrom ? p : rvec)[elements - 1]);
            rvec[elements - 1] = rl;
            acc = fma(rl, rl, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) partials[ck.chunk] = acc;
    }
}

// ---------------------------------------------------------------------------------
// Iteration 0's block SpMV of a solve whose p0 is b itself (cg_slab.hpp, LoopShape::b_is_p0): stencil5_rowlds_block_kernel on
// x = b, over the same block tiles, tile -> XCD runs, block map and p.Ap partial slots, that also sums b . b (kSelf of the shared
// pieces) into the same slot of `self_partials`. With r0 = b bit for bit both sums keep every bit that the launch of the initial
// residual followed by the block kernel gives; the values are in registers here anyway. A kernel of its own, first in its solve
// (no skip flag): the in-loop instances keep their code. kStoreAp = false (LoopShape::first_recomputed): the fast path leaves y
// alone and writes only the two partials; the other path stores A b on its rows as ever.
// ---------------------------------------------------------------------------------
template <int kRows, bool kStoreAp = true>
__global__ __launch_bounds__(64) void stencil5_first_block_kernel(
    SlabCsr m, const double* __restrict__ x, double* __restrict__ y, double alpha, int gi_lo, int gi_hi, int gfirst, int col_tiles,
    int total_blocks, int run, int reverse, double* __restrict__ dot_partials, double* __restrict__ self_partials,
    const unsigned char* __restrict__ block_map, SymPlanes sp) {
    constexpr int kFastDoubles = kRows * kRowDoubles, kOneRowDoubles = 5 * kLdsTileCols + kRowDoubles;
    __shared__ double lds[kFastDoubles > kOneRowDoubles ? kFastDoubles : kOneRowDoubles];
    const int block = rowlds_tile_of_block((int)blockIdx.x, run, total_blocks, reverse);
    if (block < 0) return;
    const BlockTile t = block_tile_at(block, col_tiles, gi_lo, kRows);
    const int lane = (int)threadIdx.x;
    const int n = m.grid_size;
    const int fast = (int)block_map[block];  // requested in front of the x loads and tested behind them
    // b has no halo rows: the rows of x that exist are the slab's own
    const int row_lo = -(m.halo_before / n), row_hi = (m.n_local + m.halo_after) / n;
    double xv[kRows + 2][2], xo[kRows];
    block_load_rows<kRows>(x, n, t.li0, t.j0, lane, row_lo, row_hi, xv, xo);
    if (__builtin_amdgcn_readfirstlane(fast) != 0) {
        block_rows_to_lds<kRows>(xv, lds, lane);
        wave_lds_sync();
        block_fast_sums<kRows, kStoreAp, true>(xv, xo, lds, n, t, lane, y, alpha, gi_lo, col_tiles, dot_partials, self_partials, sp);
    } else {
        rowlds_block_slow_rows<true>(m, x, y, alpha, gi_lo, gi_hi, gfirst, col_tiles, t, kRows, lane, 0, lds, dot_partials, self_partials, sp);
    }
}

// The block map of one launch range [gi_lo, gi_hi) (stencil5_rowlds_block_kernel): one thread per block tile.
__global__ __launch_bounds__(kBlock) void block_map_kernel(const unsigned char* __restrict__ cls, int col_tiles, int gi_lo, int gi_hi,
                                                           int block_rows, int total_blocks, unsigned char* __restrict__ out) {
    const int block = (int)(blockIdx.x * (unsigned)kBlock + threadIdx.x);
    if (block >= total_blocks) return;
    const BlockTile t = block_tile_at(block, col_tiles, gi_lo, block_rows);
    const int li0 = t.li0, col_tile = t.col_tile;
    bool fast = li0 + block_rows <= gi_hi;
    for (int r = 0; fast && r < block_rows; ++r) fast = cls[(long long)(li0 + r) * col_tiles + col_tile] == 1;
    out[block] = fast ? 1 : 0;
}

// f(std::integral_constant<int, R>, std::bool_constant<flag>) with R = the plan's grid rows per block tile (4, anything else is 8):
// the four instances each block-tile kernel has.
template <class F>
void dispatch_block(int block_rows, bool flag, F&& f) {
    if (block_rows == 4 && flag) f(std::integral_constant<int, 4>{}, std::true_type{});
    else if (block_rows == 4) f(std::integral_constant<int, 4>{}, std::false_type{});
    else if (flag) f(std::integral_constant<int, 8>{}, std::true_type{});
    else f(std::integral_constant<int, 8>{}, std::false_type{});
}

}  // namespace

// the block kernel over the plan's block tiles (the in-loop SpMV of a solver slab; launch_stencil5_spmv decides)
void launch_rowlds_block(const SlabCsr& m, const Stencil5Plan& p, const double* x, double* y, double alpha, double* d_dot_partials,
                         const int* d_skip_flag, bool reverse, hipStream_t stream, const SymPlanes& sp, bool ap_not_stored) {
    const int blocks = rowlds_block_tiles(p);
    const dim3 grid((unsigned)xcd_padded_grid(blocks, p.xcd_run));
    const int gfirst = m.row_offset / m.grid_size;
    dispatch_block(p.block_rows, !ap_not_stored, [&](auto rows, auto store) {
        hipLaunchKernelGGL((stencil5_rowlds_block_kernel<decltype(rows)::value, decltype(store)::value>), grid, dim3(64), 0, stream, m, x, y, alpha,
                           p.gi_lo, p.gi_hi, gfirst, p.row_blocks, blocks, p.xcd_run, reverse ? 1 : 0, d_dot_partials, d_skip_flag, p.block_map, sp);
    });
}

int rowlds_block_tiles(const Stencil5Plan& p) {
    if (p.variant != Stencil5Variant::RowLds || p.block_rows <= 0 || p.gi_hi <= p.gi_lo) return 0;
    return (p.gi_hi - p.gi_lo + p.block_rows - 1) / p.block_rows * p.row_blocks;
}

void launch_block_map(const unsigned char* cls, const Stencil5Plan& p, unsigned char* out, hipStream_t stream) {
    const int blocks = rowlds_block_tiles(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(block_map_kernel, dim3((unsigned)((blocks + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, cls, p.row_blocks, p.gi_lo, p.gi_hi, p.block_rows,
                       blocks, out);
}

int launch_stencil5_direction_spmv(const SlabCsr& m, const Stencil5Plan& p, const DirectionSpmv& d, double* y, double alpha,
                                   double* d_dot_partials, bool reverse, hipStream_t stream, const SymPlanes& sp) {
    const int blocks = rowlds_block_tiles(p);
    if (blocks <= 0 || p.block_map == nullptr || d_dot_partials == nullptr || sp.cls == nullptr || (d.slow_count > 0 && d.slow_list == nullptr)) {
        fprintf(stderr, "[spmv] the direction update inside the SpMV exists for row-lds plans with a block map only\n");
        exit(EXIT_FAILURE);
    }
    const dim3 grid((unsigned)xcd_padded_grid(blocks, p.xcd_run));
    const int gfirst = m.row_offset / m.grid_size;
    dispatch_block(p.block_rows, !d.ap_not_stored, [&](auto rows, auto store) {
        hipLaunchKernelGGL((stencil5_direction_block_kernel<decltype(rows)::value, decltype(store)::value>), grid, dim3(64), 0, stream, m, d.s,
                           d.iteration, d.fma_form ? 1 : 0, d.r, d.p_in, d.p_out, y, alpha, p.gi_lo, p.gi_hi, p.row_blocks, blocks, p.xcd_run,
                           reverse ? 1 : 0, d_dot_partials, p.block_map, sp);
    });
    if (d.slow_count > 0)
        hipLaunchKernelGGL(stencil5_block_list_kernel, dim3((unsigned)d.slow_count), dim3(64), 0, stream, m, d.s, d.iteration, d.p_out, y, alpha,
                           p.gi_lo, p.gi_hi, gfirst, p.row_blocks, p.block_rows, d.slow_list, d_dot_partials, sp);
    return p.partials;
}

int launch_cg_update_r_recompute(const SlabCsr& m, const Stencil5Plan& p, const CgScalars* s, const double* p_new, const double* Ap, double* r,
                                 double* partials, const unsigned char* row_fast, bool reverse, hipStream_t stream, const SymPlanes& sp, bool r_is_p) {
    const int blocks = rowlds_block_tiles(p);
    if (blocks <= 0 || row_fast == nullptr || partials == nullptr || p.first_row != 0 || p.last_row != m.n_local || m.halo_before != 0 ||
        m.halo_after != 0) {
        fprintf(stderr, "[spmv] the recomputing r update exists for whole-slab row-lds plans with a block map on slabs without halo rows only\n");
        exit(EXIT_FAILURE);
    }
    const dim3 grid((unsigned)xcd_padded_grid(blocks, p.xcd_run));
    const int n = m.grid_size;
    dispatch_block(p.block_rows, r_is_p, [&](auto rows, auto from) {
        hipLaunchKernelGGL((cg_update_r_recompute_kernel<decltype(rows)::value, decltype(from)::value>), grid, dim3(64), 0, stream,
                           (size_t)m.n_local, n, m.n_local / n, s, p_new, Ap, r, partials, p.row_blocks, blocks, p.xcd_run, reverse ? 1 : 0, row_fast,
                           sp);
    });
    return (int)slab::chunk_count((size_t)m.n_local);
}

int launch_stencil5_first_spmv(const SlabCsr& m, const Stencil5Plan& p, const double* b, double* y, double alpha, double* d_dot_partials,
                               double* self_partials, bool reverse, hipStream_t stream, const SymPlanes& sp, bool ap_not_stored) {
    const int blocks = rowlds_block_tiles(p);
    if (blocks <= 0 || p.block_map == nullptr || d_dot_partials == nullptr || self_partials == nullptr || sp.cls == nullptr || m.halo_before != 0 ||
        m.halo_after != 0) {
        fprintf(stderr, "[spmv] the first SpMV on b exists for row-lds plans with a block map on slabs without halo rows only\n");
        exit(EXIT_FAILURE);
    }
    const dim3 grid((unsigned)xcd_padded_grid(blocks, p.xcd_run));
    const int gfirst = m.row_offset / m.grid_size;
    dispatch_block(p.block_rows, !ap_not_stored, [&](auto rows, auto store) {
        hipLaunchKernelGGL((stencil5_first_block_kernel<decltype(rows)::value, decltype(store)::value>), grid, dim3(64), 0, stream, m, b, y, alpha,
                           p.gi_lo, p.gi_hi, gfirst, p.row_blocks, blocks, p.xcd_run, reverse ? 1 : 0, d_dot_partials, self_partials, p.block_map, sp);
    });
    return p.partials;
}

}  // namespace spmv_amd
