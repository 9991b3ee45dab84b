// multigrid3d_device.hpp -- the device helpers the 3-D multigrid kernels of multigrid3d.hip (one vector) and multigrid3d_multi.hip (a
// block of up to 8) share: a 7-point row sum from the wave-private LDS strip of the row's coefficients, the loads of one grid row's
// tile of coefficients, and the aggregate of a flat fine row. Unnamed namespace: each of the two translation units gets its own copy
// under the name it had when multigrid3d.hip held it alone.
#pragma once

#include <hip/hip_runtime.h>

namespace {

constexpr int kStripCols = 128;  // fine columns of one residual-restriction tile (kTileCols of both files)

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

__device__ __forceinline__ double coarse_at3d(const double* __restrict__ ec, unsigned flat, unsigned n, unsigned nc) {
    const unsigned g = flat / n, j = flat - g * n;  // g = k n + i
    const unsigned k = g / n, i = g - k * n;
    return ec[((size_t)(k >> 1) * nc + (i >> 1)) * nc + (j >> 1)];
}

}  // namespace
