// multigrid_device.hpp -- the device helper the residual-restriction kernels of multigrid.hip (one vector) and multigrid_multi.hip
// (a block of up to 8) share: a row sum from the wave-private LDS strip of the row's coefficients. Unnamed namespace: each of the two
// translation units gets its own copy under the name it had when multigrid.hip held it alone.
#pragma once

#include <hip/hip_runtime.h>

#include "stencil_row_device.hpp"

namespace {

// the row sum at column j from the strip slots of that row (v = strip + 5 (j - j0)), through stencil5_row's chains
__device__ __forceinline__ double strip_row(const double* __restrict__ v, int j, int n, double xw, double xc, double xe, double xn, double xs) {
    using spmv_amd::stencil5_row;
    if (j > 0 && j < n - 1) return stencil5_row(j, n, v[1], xw, v[2], xc, v[3], xe, v[0], xn, v[4], xs);  // [N,W,C,E,S]
    if (j == 0) return stencil5_row(j, n, 0.0, xw, v[2], xc, v[3], xe, v[1], xn, v[4], xs);                // [N,C,E,S] at 1..4
    return stencil5_row(j, n, v[1], xw, v[2], xc, 0.0, xe, v[0], xn, v[3], xs);                            // [N,W,C,S]
}

}  // namespace
