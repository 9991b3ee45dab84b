// multigrid_multi_device.hpp -- the device helpers the batched multigrid kernels of multigrid_multi.hip (the 2-D hierarchy) and
// multigrid3d_multi.hip (the 3-D one) share: the test of the column records, runs of consecutive doubles in 16-byte pieces where the
// address allows, and the flat walk's units. Unnamed namespace: each translation unit gets its own copy under the name it had when
// multigrid_multi.hip held it alone.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "multi_rhs.hpp"
#include "stream_device.hpp"

namespace {

using spmv_amd::d2;
using spmv_amd::PcgMultiColumn;

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
