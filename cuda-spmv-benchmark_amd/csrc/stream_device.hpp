// stream_device.hpp -- the small device helpers every streaming and reducing kernel of the library is written with.
#pragma once

#include <hip/hip_runtime.h>

namespace spmv_amd {

typedef double d2 __attribute__((ext_vector_type(2)));  // one 16-byte access

// Sum over the 64 lanes of a wavefront (fixed tree); the total is in lane 0.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// A scalar a solver may divide by: not zero and finite (else the iteration is a breakdown).
__device__ __forceinline__ bool usable(double v) { return v != 0.0 && isfinite(v); }

// 16-byte accesses of streams that are read / written once per pass
__device__ __forceinline__ d2 load_once(const double* __restrict__ base, size_t pair) {
    return __builtin_nontemporal_load(reinterpret_cast<const d2*>(base) + pair);
}
__device__ __forceinline__ void store_once(double* __restrict__ base, size_t pair, d2 v) {
    __builtin_nontemporal_store(v, reinterpret_cast<d2*>(base) + pair);
}

}  // namespace spmv_amd
