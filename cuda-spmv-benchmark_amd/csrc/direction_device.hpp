// direction_device.hpp -- the CG direction update p' = r + beta p as one expression, for every kernel that evaluates it: the
// streaming updates of cg_kernels.hip and the block SpMV that recomputes p' in registers (stencil5_block_kernels.hip,
// stencil5_direction_block_kernel). Both translation units must round it the same way, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

namespace spmv_amd {

// The direction update p' = r + beta p exists in two roundings upstream: the multi-GPU solver's axpby_kernel
// evaluates 1.0*r + beta*p, i.e. fma(1.0, r, beta*p) with beta*p rounded first (cg_solver_mgpu_partitioned.cu:136-140,
// :682), the single-GPU device solver's update_p_kernel evaluates r + beta*p as one fma(beta, p, r)
// (cg_solver.cu:90-95). fma_form selects the second; each solver keeps its own reference's arithmetic.
__device__ __forceinline__ double direction(double r, double beta, double p, int fma_form) {
    return fma_form ? fma(beta, p, r) : fma(1.0, r, beta * p);
}

}  // namespace spmv_amd
