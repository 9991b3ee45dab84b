// amg_multi.hip -- the device side of the batched multigrid cycle on an aggregation AMG hierarchy of "cusparse-csr" (DESIGN.md section 26;
// include/spmv_amd/api.h states the algebra under spmv_amd_precond_create_amg_multi): the two launches an AMG level adds to
// multigrid_multi.hip's cycle, on block vectors of up to 8 row-interleaved columns (multi_rhs.hpp). The hierarchy is amg.hip's, the
// cycle, term 0 and the step kernel are multigrid_multi.hip's and pcg_multi.hip's; a level's block product is launch_spmm on the level's
// "spmm/csr" plan.
//   amg_residual_restrict_multi_kernel<K>  r_c[I][j] = ((t_m0 + t_m1) + ...) per column over the members of I in ascending order,
//                                          t = fma(-1.0, s, r), s the row's sequential fma chain: ONE launch, A z and r - A z never
//                                          stored; row_ptr, col_idx, values and the member index read once for all K columns
//   amg_prolong_correct_multi_kernel<K>    z[i][j] = fma(2.0, e_c[agg[i]][j], z[i][j]), flat over rows x columns
// Per column every result has the bits of amg.hip's single-vector launch on that column alone. -ffp-contract=off: the only fused
// multiply-adds are the explicit ones. Every kernel reads the column records first and returns when no column is running (null records:
// all are); a stopped column beside running ones is computed like them.
// Indices: a row index times K is formed in 64 bits everywhere.
#include <stdint.h>

#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "multigrid.hpp"
#include "multigrid_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

namespace spmv_amd {
namespace {

constexpr int kWave = 64;
constexpr int kGroup = 8;  // lanes per aggregate: eight aggregates per wave, as in amg.hip

// A row's K columns, p = block + row * K. Even K: 16-byte accesses -- the blocks are 16-byte aligned then (api.h; the level vectors are
// allocations), so every row's run is; odd K: 8-byte accesses. No test of the address: the lanes of a wave gather different rows.
template <int K>
__device__ __forceinline__ void load_cols(const double* __restrict__ p, double (&o)[K]) {
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int q = 0; q < K; q += 2) {
            const d2 t = *reinterpret_cast<const d2*>(p + q);
            o[q] = t.x, o[q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q) o[q] = p[q];
    }
}

template <int K>
__device__ __forceinline__ void store_cols(double* __restrict__ p, const double (&v)[K]) {  // plain: the next level reads it at once
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int q = 0; q < K; q += 2) {
            d2 t;
            t.x = v[q], t.y = v[q + 1];
            *reinterpret_cast<d2*>(p + q) = t;
        }
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q) p[q] = v[q];
    }
}

// ---- residual + restriction in one launch, K columns ----
// The shape is amg_residual_restrict_kernel's (amg.hip): one-wave workgroups, eight lanes per aggregate, the round count the wave's
// maximum so that every __shfl sits in uniform control flow, a lane without a row skipped by count and not by value. A lane keeps K
// chain accumulators for its member row: per entry it loads the value and the column once and reads the contiguous run
// Z[col * K .. col * K + K). Behind a round the eight lanes' K values of t travel by shuffle and are added in member order into K
// accumulators; lane 0 of the group stores the run rc[I * K ..). An aggregate of thousands of members loops. No LDS, no scratch: all K
// columns at once fit the registers at every K (DESIGN.md section 26 has the compiler's figures), so the row is walked once.
// Bytes per fine row of q entries: 12 q + 12 shared (matrix, both ends of the row pointer, the member index) + 4 per aggregate, and per
// column 16 (r, unique z) + 8 per aggregate.
template <int K>
__global__ __launch_bounds__(kWave) void amg_residual_restrict_multi_kernel(SlabCsr m, int coarse_rows, const int* __restrict__ agg_ptr,
                                                                            const int* __restrict__ members,
                                                                            const PcgMultiColumn* __restrict__ cols,
                                                                            const double* __restrict__ z, const double* __restrict__ r,
                                                                            double* __restrict__ rc) {
    if (!any_running<K>(cols)) return;  // uniform over the launch
    const int lane = (int)threadIdx.x;
    const int sub = lane & (kGroup - 1), first = lane & ~(kGroup - 1);
    const long long I = (long long)blockIdx.x * (kWave / kGroup) + (lane / kGroup);
    const bool live = I < coarse_rows;
    const int m0 = live ? agg_ptr[I] : 0, m1 = live ? agg_ptr[I + 1] : 0;
    int rounds = (m1 - m0 + kGroup - 1) / kGroup;
#pragma unroll
    for (int off = kWave / 2; off >= kGroup; off >>= 1) {  // the wave's maximum: the lanes of a group agree already
        const int other = __shfl_xor(rounds, off);
        rounds = other > rounds ? other : rounds;
    }
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int round = 0; round < rounds; ++round) {
        const int begin = m0 + kGroup * round;
        const int have = m1 - begin;  // members of this round: may be <= 0 in a group that is done
        double t[K];
#pragma unroll
        for (int j = 0; j < K; ++j) t[j] = 0.0;
        if (sub < have) {
            const long long row = members[begin + sub];
            double s[K], rr[K];
#pragma unroll
            for (int j = 0; j < K; ++j) s[j] = 0.0;
            const int e1 = m.row_ptr[row + 1];
            for (int e = m.row_ptr[row]; e < e1; ++e) {
                const double v = m.values[e];
                double zc[K];
                load_cols<K>(z + (long long)m.col_idx[e] * K, zc);
#pragma unroll
                for (int j = 0; j < K; ++j) s[j] = fma(v, zc[j], s[j]);
            }
            load_cols<K>(r + row * K, rr);
#pragma unroll
            for (int j = 0; j < K; ++j) t[j] = fma(-1.0, s[j], rr[j]);
        }
#pragma unroll
        for (int q = 0; q < kGroup; ++q) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double tq = __shfl(t[j], first + q);
                const double sum = (round == 0 && q == 0) ? tq : acc[j] + tq;
                acc[j] = q < have ? sum : acc[j];
            }
        }
    }
    if (live && sub == 0) store_cols<K>(rc + I * K, acc);
}

// ---- prolongation + correction: z[i][j] = fma(2.0, e_c[agg[i]][j], z[i][j]), z in place; multigrid_multi.hip's flat walk, the
// aggregate read from the map once per row-unit; the store is plain: the post-smoother's SpMM reads it ----
template <int K>
__global__ __launch_bounds__(kFlat) void amg_prolong_correct_multi_kernel(long long rows, const int* __restrict__ agg,
                                                                          const PcgMultiColumn* __restrict__ cols,
                                                                          const double* __restrict__ ec, double* __restrict__ z) {
    constexpr int V = FlatWalk<K>::V, U = FlatWalk<K>::P;
    if (!any_running<K>(cols)) return;
    const long long row0 = (long long)blockIdx.x * kFlat;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kFlat * i;
        const int t = f / U, col0 = (f - t * U) * V;
        const long long row = row0 + t;
        if (row >= rows) continue;
        const long long coarse = agg[row];
        double zv[V], ev[V];
        load_unit<V>(z + row * K + col0, zv);
        load_unit<V>(ec + coarse * K + col0, ev);
#pragma unroll
        for (int q = 0; q < V; ++q) zv[q] = fma(2.0, ev[q], zv[q]);
        store_unit<V>(z + row * K + col0, zv);
    }
}

}  // namespace

// ---- the launches: the batched cycle calls these, and so does the LAB build's spmv_amd_amg_multi_stage ----
void launch_amg_residual_restrict_multi(int k, const SlabCsr& m, int coarse_rows, const int* agg_ptr, const int* members,
                                        const PcgMultiColumn* cols, const double* Z, const double* R, double* Rc) {
    if (coarse_rows <= 0) return;
    const unsigned grid = (unsigned)(((long long)coarse_rows + kWave / kGroup - 1) / (kWave / kGroup));
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((amg_residual_restrict_multi_kernel<decltype(K)::value>), dim3(grid), dim3(kWave), 0, kBatchStream, m, coarse_rows,
                           agg_ptr, members, cols, Z, R, Rc);
    });
}

void launch_amg_prolong_correct_multi(int k, size_t rows, const int* agg, const PcgMultiColumn* cols, const double* Ec, double* Z) {
    if (rows == 0) return;
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((amg_prolong_correct_multi_kernel<decltype(K)::value>), dim3((unsigned)((rows + kFlat - 1) / kFlat)), dim3(kFlat), 0,
                           kBatchStream, (long long)rows, agg, cols, Ec, Z);
    });
}

}  // namespace spmv_amd

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_amg_multi_stage(const char* stage, int k, SpmvAmdAmgStageArgs* a) {
    if (k < 1 || k > spmv_amd::kMaxRhs) {  // before any HIP call, like the body's own checks
        fprintf(stderr, "[PCG] amg: stage: k is not 1 to 8\n");
        return 1;
    }
    return spmv_amd::amg_stage(stage, k, a);  // amg.hip: the one body of both stage hooks
}
#endif  // SPMV_AMD_LAB
