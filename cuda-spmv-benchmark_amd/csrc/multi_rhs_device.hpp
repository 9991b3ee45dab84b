// multi_rhs_device.hpp -- the device helpers the batched solvers share (cg_multi.hip: batched CG; pcg_multi.hip: batched
// preconditioned CG; bicgstab_multi.hip: batched BiCGSTAB): a row's k values as 16-byte accesses, the flat row x column walk of a
// workgroup, one unit of a stream touched once per pass, the per-column dot partials of a workgroup's 256 rows for one or two values,
// and the first stage of the two-stage per-column sum (its geometry: slices_for, multi_rhs.hpp).
// Everything sits in an unnamed namespace: each translation unit gets its own copy under the names it had when
// cg_multi.hip held them alone, so moving them here changes no kernel's code or symbol (profiles/r25_pcg_multi_isa_identity.txt).
#pragma once

#include <hip/hip_runtime.h>

#include "multi_rhs.hpp"
#include "reduce_device.hpp"
#include "stream_device.hpp"

namespace {

using namespace spmv_amd;

constexpr int kBlock = kReduceBlock;  // 256: the vector kernels' workgroup and the width of block_tree (reduce_device.hpp)
constexpr int kSlice = kReduceSlice;  // partials one workgroup of the first reduction stage sums: 16 per thread
static_assert(kSlice == kBlock * 16, "slices_for (multi_rhs.hpp) and the first reduction stage agree on the slice");

template <int K>
__device__ __forceinline__ void load_row(const double* __restrict__ p, double (&o)[K]) {
    if constexpr (K % 2 == 0) {  // workspace vectors: hipMalloc'd, rows of 8k bytes
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

template <int K>
__device__ __forceinline__ void store_row(double* __restrict__ p, const double (&v)[K]) {
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int i = 0; i < K / 2; ++i) {
            d2 t;
            t.x = v[2 * i], t.y = v[2 * i + 1];
            reinterpret_cast<d2*>(p)[i] = t;
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) p[i] = v[i];
    }
}

// One partial per column of the workgroup's 256 rows: wave trees, then the four wave sums in wave order (the shape of the
// SpMM's partials; independent of k and of the column's slot).
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

// The vector kernels walk their workgroup's 256 rows x k columns FLAT (as the row-lds SpMM does, spmm_kernels.hip): unit
// f = threadIdx.x + 256 i (i < P) is row f / P, columns (f % P) * V ... + V - 1, with V = 2 for even k (16-byte accesses), 1
// else, P = k / V -- every access of one instruction is one contiguous run. Dot products go through LDS back to thread = row
// and into block_partials: per column, the same shape whatever k is.
template <int K>
struct Flat {
    static constexpr int V = K % 2 == 0 ? 2 : 1;
    static constexpr int P = K / V;
};

// Thread = row again: the k products of the thread's row from LDS (every thread of the workgroup calls it: it has a barrier).
template <int K>
__device__ __forceinline__ void products_to_rows(const double* prod, double (&d)[K]) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) d[q] = prod[threadIdx.x * K + q];
}

// One unit (V = 1 or 2 values) of a stream that is read / written once per pass
template <int V>
__device__ __forceinline__ void load_unit_once(const double* __restrict__ p, double (&o)[V]) {
    if constexpr (V == 2) {
        const d2 t = __builtin_nontemporal_load(reinterpret_cast<const d2*>(p));
        o[0] = t.x, o[1] = t.y;
    } else {
        o[0] = __builtin_nontemporal_load(p);
    }
}
template <int V>
__device__ __forceinline__ void store_unit_once(double* __restrict__ p, const double (&v)[V]) {
    if constexpr (V == 2) {
        d2 t;
        t.x = v[0], t.y = v[1];
        __builtin_nontemporal_store(t, reinterpret_cast<d2*>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// The partials of one or two values from the units' products: value 0 (in prod already) at partials[j * count + blk], value 1
// (second[], this thread's units in walk order) at partials[(K + j) * count + blk] through the same LDS array. Every thread of the
// workgroup calls it.
template <int K>
__device__ __forceinline__ void unit_partials(double* prod, bool first, const double (&second)[K], bool with_second,
                                              double* __restrict__ partials, long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    double d[K];
    if (first) {
        products_to_rows<K>(prod, d);
        block_partials<K>(d, partials, count, blockIdx.x);
    }
    if (!with_second) return;
    __syncthreads();  // every thread has read its row of prod, and threads < K the wave sums
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = second[i * V + q];
    }
    products_to_rows<K>(prod, d);
    block_partials<K>(d, partials + (long long)K * count, count, blockIdx.x);
}

// Stage 1: workgroup (s, j) sums partials[j * count + s * kSlice ...] (each thread its strided share in ascending order, then
// a fixed tree) into slices[j * slice_count + s].
__global__ __launch_bounds__(kBlock) void multi_reduce_slices_kernel(const double* __restrict__ partials, long long count, int slice_count,
                                                                    double* __restrict__ slices) {
    __shared__ double s[kBlock];
    const int j = (int)blockIdx.y, sl = (int)blockIdx.x;
    const double* __restrict__ src = partials + (long long)j * count;
    const long long lo = (long long)sl * kSlice, hi = lo + kSlice < count ? lo + kSlice : count;
    double acc = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += kBlock) acc += src[i];
    block_tree(acc, s);
    if (threadIdx.x == 0) slices[(long long)j * slice_count + sl] = s[0];
}

}  // namespace
