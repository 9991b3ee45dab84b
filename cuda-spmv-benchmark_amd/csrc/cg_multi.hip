// cg_multi.hip -- batched CG: up to 8 independent systems A x_j = b_j solved together, one matrix pass per iteration.
//
// Each column is its own CG solve -- own alpha, beta, stopping test, history and iteration count, the algebra of
// cg_solve_device (reference src/solvers/cg_solver.cu:436-706, oracle_cg's device form). The only thing the columns share is
// the SpMM (spmm_kernels.hip), which reads the coefficients once for all of them. Not block CG: no shared Krylov space.
//
// One iteration, five kinds of launch on the default stream (block vectors interleaved, multi_rhs.hpp):
//   AP = A P with the per-column p.Ap partials | sum + pAp step (active = !done, alpha = rr_old / pAp) |
//   R -= alpha AP with the r.r partials | sum + rr step (residual, history, verdict, beta) |
//   X += alpha P, then P = R + beta P unless the column converged in this iteration
// then one small blocking read of the k column states (the stopping test; ~10 us against milliseconds of work). A converged
// column is frozen: every kernel leaves its X, R, P, history and iteration count alone from the next iteration on.
// Bytes per interior row and iteration, per system: (40 + 80 k) / k.
// No run-ahead, no direction ring, no status protocol: that machinery (cg_slab.hip) buys microseconds per iteration of a
// single solve; here an iteration is k times longer.
// This file: the kernels, their launchers, the loop and the LAB build's stage hook. What surrounds the loop -- workspace, argument
// checks, upload and download, histories, statistics, print-out -- is multi_solve.hpp, shared with pcg_multi.hip.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "multi_rhs_device.hpp"
#include "multi_solve.hpp"
#include "reduce_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr const char* kTag = "CG-MULTI";
constexpr const char* kOperandTag = "multi-rhs";  // nrhs and the operator: refused in the words of the operand entry points (spmm_kernels.hip)

// load_row, store_row, block_partials, Flat, products_to_rows, multi_reduce_slices_kernel: multi_rhs_device.hpp

// R = b - A x0 (R holds b on entry: axpby_kernel(1.0, b, -1.0, Ap), cg_solver.cu:48-54), P = R, partials of r.r.
template <int K>
__global__ __launch_bounds__(kBlock) void multi_init_residual_kernel(long long n, const double* __restrict__ AP, double* __restrict__ R,
                                                                    double* __restrict__ P, double* __restrict__ partials, long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    __shared__ double prod[kBlock * K];
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        double r[V] = {};
        if (row0 + t < n) {
            const long long at = (row0 + t) * K + col0;
            double ap[V];
            load_row<V>(AP + at, ap);
            load_row<V>(R + at, r);
#pragma unroll
            for (int q = 0; q < V; ++q) r[q] = fma(1.0, r[q], -1.0 * ap[q]);
            store_row<V>(R + at, r);
            store_row<V>(P + at, r);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q];
    }
    double d[K];
    products_to_rows<K>(prod, d);
    block_partials<K>(d, partials, count, blockIdx.x);
}

// r = fma(-alpha, Ap, r) for the active columns (cg_solver.cu:59-74), partials of r.r.
template <int K>
__global__ __launch_bounds__(kBlock) void multi_update_r_kernel(long long n, const MultiColumn* __restrict__ cols, const double* __restrict__ AP,
                                                               double* __restrict__ R, double* __restrict__ partials, long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    __shared__ double prod[kBlock * K];
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        double r[V] = {};
        if (row0 + t < n) {
            const long long at = (row0 + t) * K + col0;
            double ap[V];
            load_row<V>(AP + at, ap);
            load_row<V>(R + at, r);
#pragma unroll
            for (int q = 0; q < V; ++q)
                if (cols[col0 + q].active) r[q] = fma(-cols[col0 + q].alpha, ap[q], r[q]);
            store_row<V>(R + at, r);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q];
    }
    double d[K];
    products_to_rows<K>(prod, d);
    block_partials<K>(d, partials, count, blockIdx.x);
}

// x = fma(alpha, p, x) for the active columns; then p = fma(beta, p, r) (update_p_kernel, cg_solver.cu:90-95) for those that
// did not converge in this iteration.
template <int K>
__global__ __launch_bounds__(kBlock) void multi_update_xp_kernel(long long n, const MultiColumn* __restrict__ cols, const double* __restrict__ R,
                                                                double* __restrict__ P, double* __restrict__ X) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        if (row0 + t >= n) continue;
        const long long at = (row0 + t) * K + col0;
        double x[V], p[V], r[V];
        load_row<V>(X + at, x);
        load_row<V>(P + at, p);
        load_row<V>(R + at, r);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const MultiColumn& c = cols[col0 + q];
            if (c.active) {
                x[q] = fma(c.alpha, p[q], x[q]);
                if (!c.done) p[q] = fma(c.beta, p[q], r[q]);
            }
        }
        store_row<V>(X + at, x);
        store_row<V>(P + at, p);
    }
}

// Stage 2 + the scalar step of column j (workgroup j). which: 0 = initial residual, 1 = pAp, 2 = r.r.
__global__ __launch_bounds__(kBlock) void multi_reduce_step_kernel(const double* __restrict__ slices, int slice_count, int which, double tol,
                                                                  MultiColumn* __restrict__ cols, double* __restrict__ hist, int hist_cap) {
    __shared__ double s[kBlock];
    const int j = (int)blockIdx.x;
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < slice_count; i += kBlock) acc += slices[(long long)j * slice_count + i];
    block_tree(acc, s);
    if (threadIdx.x != 0) return;
    const double total = s[0];
    MultiColumn& c = cols[j];
    double* h = hist + (long long)j * hist_cap;
    if (which == 0) {
        c.rr_old = total;
        c.b_norm = sqrt(total);
        c.residual = c.b_norm;
        c.alpha = c.beta = c.pAp = 0.0;
        c.active = 0, c.done = 0, c.iterations = 0;
        h[0] = c.b_norm;
    } else if (which == 1) {
        c.active = c.done ? 0 : 1;
        if (c.active) {
            c.pAp = total;
            c.alpha = c.rr_old / total;
        }
    } else if (c.active) {
        const double res = sqrt(total);
        c.iterations += 1;
        if (c.iterations < hist_cap) h[c.iterations] = res;
        c.residual = res;
        if (res / c.b_norm < tol) {
            c.done = 1;
        } else {
            c.beta = total / c.rr_old;
            c.rr_old = total;
        }
    }
}

template <int K>
void launch_vec(int which, long long n, const MultiColumn* cols, double* X, double* R, double* P, const double* AP, double* partials,
                long long count) {
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (which == 0) hipLaunchKernelGGL((multi_init_residual_kernel<K>), grid, block, 0, kBatchStream, n, AP, R, P, partials, count);
    else if (which == 1) hipLaunchKernelGGL((multi_update_r_kernel<K>), grid, block, 0, kBatchStream, n, cols, AP, R, partials, count);
    else hipLaunchKernelGGL((multi_update_xp_kernel<K>), grid, block, 0, kBatchStream, n, cols, R, P, X);
}

void launch_vector_step(int k, int which, long long n, const MultiColumn* cols, double* X, double* R, double* P, const double* AP,
                        double* partials, long long count) {
    auto launch = [&](auto K) { launch_vec<decltype(K)::value>(which, n, cols, X, R, P, AP, partials, count); };
    if (!dispatch_k(k, launch)) launch(std::integral_constant<int, kMaxRhs>{});
}

// The two reduction launches behind every dot product: k x slices_for(count) slice sums, then per column their sum and the
// scalar step `which`. slices: k x slices_for(count) doubles.
void launch_reduce(int k, const double* partials, long long count, double* slices, int which, double tol, MultiColumn* cols, double* hist,
                   int hist_cap) {
    const int sc = slices_for(count);
    hipLaunchKernelGGL(multi_reduce_slices_kernel, dim3((unsigned)sc, (unsigned)k), dim3(kBlock), 0, kBatchStream, partials, count, sc, slices);
    hipLaunchKernelGGL(multi_reduce_step_kernel, dim3((unsigned)k), dim3(kBlock), 0, kBatchStream, slices, sc, which, tol, cols, hist, hist_cap);
}

BatchedWorkspace<MultiColumn> g_multi(1);           // one dot-product value per launch
std::vector<std::vector<double>> g_multi_history;  // of the last batched solve, per column

ColumnSummary summary_of(const MultiColumn& c) { return {c.iterations, c.done != 0, false, c.residual, c.b_norm, c.active != 0}; }

}  // namespace

namespace spmv_amd {
void release_cg_multi_workspace_locked() { g_multi.release(); }
size_t cg_multi_workspace_bytes_locked() { return g_multi.bytes(); }
}  // namespace spmv_amd

extern "C" int spmv_amd_cg_solve_device_multi(SpmvOperator* op, MatrixData* mat, int nrhs, const double* B, double* X,
                                              const CGConfig* config, CGStats* stats) {
    MultiOperand o;
    if (!check_batched_system(kTag, kOperandTag, op, mat, nrhs, B, X, config, stats, &o)) return 1;  // before the first HIP call
    const int n = mat->rows, k = nrhs;
    const CGConfig cfg = *config;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const long long vec_count = ((long long)n + kBlock - 1) / kBlock;
    const long long spmm_count = o.plan.blocks;
    BatchedWorkspace<MultiColumn>& w = g_multi;
    if (!w.ensure(kTag, n, k, device, vec_count > spmm_count ? vec_count : spmm_count, cfg.max_iters + 1, false)) return 1;
    load_block_system(w, k, n, B, X);

    std::vector<ColumnSummary> cols;
    StageTimers T(cfg.enable_detailed_timers != 0, kBatchStream);
    auto reduce = [&](long long count, int which) {
        launch_reduce(k, w.partials, count, w.slices, which, cfg.tolerance, w.cols, w.hist, w.hist_cap);
    };

    T.total.begin(kBatchStream);
    T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, w.X, w.AP, nullptr, kBatchStream); });
    T.run(&T.t_blas, [&] { launch_vector_step(k, 0, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
    T.run(&T.t_red, [&] { reduce(vec_count, 0); });
    read_columns(w, k, summary_of, cols);
    if (cfg.verbose >= 1) print_initial_residuals(kTag, cols, nullptr);
    for (int it = 0; it < cfg.max_iters && any_column_running(cols); ++it) {
        T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, w.P, w.AP, w.partials, kBatchStream); });
        T.run(&T.t_red, [&] { reduce(spmm_count, 1); });
        T.run(&T.t_blas, [&] { launch_vector_step(k, 1, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
        T.run(&T.t_red, [&] { reduce(vec_count, 2); });
        T.run(&T.t_blas, [&] { launch_vector_step(k, 2, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
        read_columns(w, k, summary_of, cols);  // synchronises: the stopping test of every column
        if (cfg.verbose >= 2) print_iteration(kTag, cols);
    }
    T.total.end(kBatchStream);
    finish_batched_solve(kTag, w, k, n, X, stats, cfg, T, T.total.elapsed_ms(), cols, g_multi_history);
    return 0;
}

extern "C" size_t spmv_amd_cg_multi_workspace_bytes(void) {
    CgWorkspaceScope scope;
    return cg_multi_workspace_bytes_locked();
}

extern "C" int spmv_amd_cg_last_history_multi(int rhs, double* out, int cap) {
    if (rhs < 0 || rhs >= (int)g_multi_history.size()) return -1;
    return copy_history(g_multi_history[(size_t)rhs], out, cap);
}

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_multi_rhs_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdMultiColumn) == sizeof(MultiColumn) && offsetof(SpmvAmdMultiColumn, rr_old) == offsetof(MultiColumn, rr_old) &&
                  offsetof(SpmvAmdMultiColumn, pAp) == offsetof(MultiColumn, pAp) && offsetof(SpmvAmdMultiColumn, alpha) == offsetof(MultiColumn, alpha) &&
                  offsetof(SpmvAmdMultiColumn, beta) == offsetof(MultiColumn, beta) && offsetof(SpmvAmdMultiColumn, b_norm) == offsetof(MultiColumn, b_norm) &&
                  offsetof(SpmvAmdMultiColumn, residual) == offsetof(MultiColumn, residual) &&
                  offsetof(SpmvAmdMultiColumn, active) == offsetof(MultiColumn, active) && offsetof(SpmvAmdMultiColumn, done) == offsetof(MultiColumn, done) &&
                  offsetof(SpmvAmdMultiColumn, iterations) == offsetof(MultiColumn, iterations),
              "lab.h's column record is the device record, field for field");

extern "C" int spmv_amd_cg_multi_stage(const char* stage, int k, SpmvAmdCgMultiStageArgs* a) {
    // argument checks: all before the first HIP call. 16: a block vector the vector kernels access in 16-byte pairs
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    enum { kSpmm, kInit, kUpdateR, kUpdateXp, kReduce } st;
    if (stage == nullptr) return refuse("no stage named (spmm, init, update_r, update_xp, reduce)"), 1;
    if (!strcmp(stage, "spmm")) st = kSpmm;
    else if (!strcmp(stage, "init")) st = kInit;
    else if (!strcmp(stage, "update_r")) st = kUpdateR;
    else if (!strcmp(stage, "update_xp")) st = kUpdateXp;
    else if (!strcmp(stage, "reduce")) st = kReduce;
    else return refuse("unknown stage (spmm, init, update_r, update_xp, reduce)"), 1;
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    MultiOperand o;
    if (st == kSpmm) {
        if (!pointer("X", a->X, 8) || !pointer("AP", a->AP, 8)) return 1;
        if (a->partials != nullptr && !pointer("partials", a->partials, 8)) return 1;
        if (a->xcd_run < 0) return refuse("xcd_run < 0"), 1;
        if (a->mode == nullptr) return refuse("no operator named"), 1;
        SpmvOperator* op = get_operator(a->mode);
        if (op == nullptr) return refuse("unknown operator"), 1;
        if (!usable_operator(kOperandTag, op, &o)) return refuse("the operator has no usable multi-RHS path"), 1;
    } else if (st == kReduce) {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 2) return refuse("which is not 0, 1 or 2"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (a->which == 0 && a->hist_cap < 1) return refuse("hist_cap < 1 for step 0, which writes the first entry"), 1;
        if (!pointer("partials", a->partials, 8) || !pointer("cols", a->cols, 8)) return 1;
        if (a->hist_cap > 0 && !pointer("hist", a->hist, 8)) return 1;
    } else {
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
        if (st != kInit && !pointer("cols", a->cols, 8)) return 1;
        if (st != kUpdateXp && (!pointer("AP", a->AP, 16) || !pointer("partials", a->partials, 8))) return 1;
        if (!pointer("R", a->R, 16)) return 1;
        if (st != kUpdateR && !pointer("P", a->P, 16)) return 1;
        if (st == kUpdateXp && !pointer("X", a->X, 16)) return 1;
    }

    MultiColumn* cols = reinterpret_cast<MultiColumn*>(a->cols);
    double* slices = nullptr;
    if (st == kSpmm) {
        SpmmPlan plan = o.plan;
        if (a->xcd_run > 0) plan.xcd_run = a->xcd_run;
        launch_spmm(plan, k, a->X, a->AP, a->partials, kBatchStream);
        a->count = plan.blocks;
    } else if (st == kReduce) {
        slices = device_alloc<double>((size_t)k * slices_for(a->count));
        launch_reduce(k, a->partials, a->count, slices, a->which, a->tol, cols, a->hist, a->hist_cap);
    } else {
        const long long n = (long long)a->n, count = (n + kBlock - 1) / kBlock;
        launch_vector_step(k, st == kInit ? 0 : st == kUpdateR ? 1 : 2, n, cols, a->X, a->R, a->P, a->AP, a->partials, count);
        a->count = count;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    device_release(slices);
    return 0;
}
#endif  // SPMV_AMD_LAB