// stencil_row_device.hpp -- what every 5-point-stencil kernel of the library (spmv_kernels.hip, stencil5_block_kernels.hip, spmm_kernels.hip) must do the
// same way, bit for bit: the fma chain of one row, the workgroup -> tile relabelling over the XCDs, the ordering of a wave's
// private LDS, and the W / E neighbour exchange through the LDS copy of a tile's x row.
//
// Arithmetic contract (numerical-semantics checklist): every multiply-add is an explicit fma() and the
// files are compiled with -ffp-contract=off, so the order and fusing of operations is exactly
//   interior stencil rows : t = vW*xW ; fma(vC,xC,t) ; fma(vE,xE,t) ; fma(vN,xN,t) ; fma(vS,xS,t)
//                           (reference src/spmv/spmv_stencil_csr_direct.cu:105-109 under nvcc -fmad)
//   every other row       : sum = 0 ; sum = fma(v[k], x[col[k]], sum) for ascending k
//                           (reference :116-119 ; cg_solver_mgpu_partitioned.cu:49-52)
// which is what oracle/spmv_oracle.c evaluates on the CPU. Columns 0 and n-1 of an interior grid row are "every other row" with
// four entries in ascending column order: N,C,E,S and N,W,C,S. The chains are written out below; the three sites that keep a copy of
// their own (the CSR strip form of rowlds_tile, ell_stencil5_kernel, the SpMM's edge-column loops) point to the record that says why
// (profiles/r14_stencil_helpers_isa_identity.txt).
#pragma once

#include <hip/hip_runtime.h>

namespace spmv_amd {

// Operands come in (coefficient, x) pairs in each chain's own evaluation order: a caller that names memory in the argument list
// then issues its loads in the order it did when the chain stood in it (an N-first signature of the interior chain reordered the
// loads of the one-thread-per-row kernels).
__device__ __forceinline__ double stencil5_interior(double vw, double xw, double vc, double xc, double ve, double xe, double vn, double xn,
                                                    double vs, double xs) {
    double sum = vw * xw;
    sum = fma(vc, xc, sum);
    sum = fma(ve, xe, sum);
    sum = fma(vn, xn, sum);
    return fma(vs, xs, sum);
}

// column 0: the CSR loop's order over [N,C,E,S], the sum started at 0
__device__ __forceinline__ double stencil5_first_column(double vn, double xn, double vc, double xc, double ve, double xe, double vs, double xs) {
    double sum = fma(vn, xn, 0.0);
    sum = fma(vc, xc, sum);
    sum = fma(ve, xe, sum);
    return fma(vs, xs, sum);
}

// column n-1: the CSR loop's order over [N,W,C,S], the sum started at 0
__device__ __forceinline__ double stencil5_last_column(double vn, double xn, double vw, double xw, double vc, double xc, double vs, double xs) {
    double sum = fma(vn, xn, 0.0);
    sum = fma(vw, xw, sum);
    sum = fma(vc, xc, sum);
    return fma(vs, xs, sum);
}

// Row at column j of an interior grid row of an n x n grid, for callers whose five coefficients have the same names in all three
// cases (the symmetric planes, the slab-wide quintuple); the CSR strip holds a 4-entry row in other slots and branches itself.
__device__ __forceinline__ double stencil5_row(int j, int n, double vw, double xw, double vc, double xc, double ve, double xe, double vn,
                                               double xn, double vs, double xs) {
    if (j > 0 && j < n - 1) return stencil5_interior(vw, xw, vc, xc, ve, xe, vn, xn, vs, xs);
    if (j == 0) return stencil5_first_column(vn, xn, vc, xc, ve, xe, vs, xs);
    return stencil5_last_column(vn, xn, vw, xw, vc, xc, vs, xs);
}

// Workgroups are dealt round-robin to the eight XCDs. This re-labels workgroup b so that each XCD works on `run` CONSECUTIVE
// tiles of every span of 8 * run (the row-lds finding, DESIGN.md section 3: with the same kernel body, which XCD touches which
// addresses is worth ~5 %). The launcher pads the grid to xcd_padded_grid(); the caller drops tiles relabelled past its total.
// A performance choice only, never a correctness input. I: the caller's index type (int, or long long where tiles can pass 2^31).
template <typename I>
__device__ __forceinline__ I xcd_run_tile(I b, I run) {
    const I span = 8 * run;
    return (b / span) * span + (b & 7) * run + ((b >> 3) % run);
}

// the grid xcd_run_tile() needs: `total` rounded up to whole spans of 8 * run
inline long long xcd_padded_grid(long long total, int run) {
    const long long span = 8LL * run;
    return (total + span - 1) / span * span;
}

// Orders a wave's accesses to LDS that only this wave touches: what its lanes wrote before is what its lanes read after (and a
// later write does not overtake an earlier read). No workgroup barrier: LDS operations of one wave retire in order; the fences
// keep the compiler from moving accesses across, at wavefront scope no cache operation is emitted.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W / E neighbours of a lane's two columns (j0 + lane, j0 + 64 + lane) of a 128-column tile, from the LDS copy of the tile's own
// x row: xrow[1 + c] = x at column j0 + c, written by the wave and ordered by wave_lds_sync() before this call. Only the tile's
// two outer neighbours come from memory: `west` is used by lane 0, `east` by lane 63 (0 where the grid row ends there). Columns
// beyond n hold 0 in the copy, exactly what an absent neighbour contributes, and the lane whose first column is n-1 takes E = 0.
__device__ __forceinline__ void tile_west_east(const double* __restrict__ xrow, int lane, int j0, int n, double west, double east,
                                               double (&xw)[2], double (&xe)[2]) {
    xw[0] = lane > 0 ? xrow[lane] : west;
    xe[0] = xrow[2 + lane];
    xw[1] = xrow[64 + lane];
    xe[1] = lane < 63 ? xrow[66 + lane] : east;
    if (j0 + lane == n - 1) xe[0] = 0.0;
}

}  // namespace spmv_amd
