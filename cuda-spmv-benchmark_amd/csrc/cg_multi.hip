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
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "multi_rhs_device.hpp"
#include "reduce_device.hpp"
#include "solve_common.hpp"
#include "stream_device.hpp"

#include "spmv_amd/lab.h"

using namespace spmv_amd;

namespace {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators

// load_row, store_row, block_partials, Flat, products_to_rows, multi_reduce_slices_kernel, slices_for: multi_rhs_device.hpp

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
    if (which == 0) hipLaunchKernelGGL((multi_init_residual_kernel<K>), grid, block, 0, kStream, n, AP, R, P, partials, count);
    else if (which == 1) hipLaunchKernelGGL((multi_update_r_kernel<K>), grid, block, 0, kStream, n, cols, AP, R, partials, count);
    else hipLaunchKernelGGL((multi_update_xp_kernel<K>), grid, block, 0, kStream, n, cols, R, P, X);
}

void launch_vector_step(int k, int which, long long n, const MultiColumn* cols, double* X, double* R, double* P, const double* AP,
                        double* partials, long long count) {
    switch (k) {
        case 1: launch_vec<1>(which, n, cols, X, R, P, AP, partials, count); break;
        case 2: launch_vec<2>(which, n, cols, X, R, P, AP, partials, count); break;
        case 3: launch_vec<3>(which, n, cols, X, R, P, AP, partials, count); break;
        case 4: launch_vec<4>(which, n, cols, X, R, P, AP, partials, count); break;
        case 5: launch_vec<5>(which, n, cols, X, R, P, AP, partials, count); break;
        case 6: launch_vec<6>(which, n, cols, X, R, P, AP, partials, count); break;
        case 7: launch_vec<7>(which, n, cols, X, R, P, AP, partials, count); break;
        default: launch_vec<8>(which, n, cols, X, R, P, AP, partials, count); break;
    }
}

// The two reduction launches behind every dot product: k x slices_for(count) slice sums, then per column their sum and the
// scalar step `which`. slices: k x slices_for(count) doubles.
void launch_reduce(int k, const double* partials, long long count, double* slices, int which, double tol, MultiColumn* cols, double* hist,
                   int hist_cap) {
    const int sc = slices_for(count);
    hipLaunchKernelGGL(multi_reduce_slices_kernel, dim3((unsigned)sc, (unsigned)k), dim3(kBlock), 0, kStream, partials, count, sc, slices);
    hipLaunchKernelGGL(multi_reduce_step_kernel, dim3((unsigned)k), dim3(kBlock), 0, kStream, slices, sc, which, tol, cols, hist, hist_cap);
}

// ---- workspace: kept between calls (like cg_solve_device's), released with it ----
struct MultiWorkspace {
    int n = 0, k = 0, device = -1;
    double *X = nullptr, *R = nullptr, *P = nullptr, *AP = nullptr;
    double* partials = nullptr;  // k x max(SpMM partials, vector partials)
    double* slices = nullptr;    // k x slices of that
    MultiColumn* cols = nullptr;
    double* hist = nullptr;      // k x hist_cap
    int hist_cap = 0;
    long long partial_cap = 0;
    void release() {
        device_release(X);
        device_release(R);
        device_release(P);
        device_release(AP);
        device_release(partials);
        device_release(slices);
        device_release(cols);
        device_release(hist);
        n = k = 0, device = -1, hist_cap = 0, partial_cap = 0;
    }
};
MultiWorkspace g_multi;
std::vector<std::vector<double>> g_multi_history;  // of the last batched solve, per column

bool fail(const char* what) {
    fprintf(stderr, "[CG-MULTI] %s\n", what);
    return false;
}

// Allocates the workspace for (n, k, partial slots) if it is not there already (sized against the free memory first).
bool ensure_workspace(int n, int k, int device, long long partial_cap, int hist_cap) {
    MultiWorkspace& w = g_multi;
    if (w.X != nullptr && (w.n != n || w.k != k || w.device != device || w.partial_cap < partial_cap)) w.release();
    if (w.X == nullptr) {
        const size_t vec = (size_t)n * k * sizeof(double);
        const size_t need = 4 * vec + (size_t)k * partial_cap * sizeof(double) + (size_t)k * slices_for(partial_cap) * sizeof(double) +
                            (size_t)k * hist_cap * sizeof(double) + ((size_t)64 << 20);
        char what[48];
        snprintf(what, sizeof what, "%d systems of %d rows", k, n);
        if (!device_has_room(need, "CG-MULTI", what)) return false;
        w.X = device_try_alloc<double>((size_t)n * k);
        w.R = device_try_alloc<double>((size_t)n * k);
        w.P = device_try_alloc<double>((size_t)n * k);
        w.AP = device_try_alloc<double>((size_t)n * k);
        w.partials = device_try_alloc<double>((size_t)k * partial_cap);
        w.slices = device_try_alloc<double>((size_t)k * slices_for(partial_cap));
        w.cols = device_try_alloc<MultiColumn>((size_t)k);
        if (!w.X || !w.R || !w.P || !w.AP || !w.partials || !w.slices || !w.cols) {
            w.release();
            return fail("the workspace could not be allocated: refused");
        }
        w.n = n, w.k = k, w.device = device, w.partial_cap = partial_cap;
    }
    if (!grow_history(w.hist, w.hist_cap, hist_cap, (size_t)k)) return fail("the history could not be allocated: refused");
    return true;
}

bool check_rhs(int nrhs) {
    if (nrhs < 1 || nrhs > kMaxRhs) {
        fprintf(stderr, "[multi-rhs] nrhs = %d: 1 to %d right-hand sides are supported\n", nrhs, kMaxRhs);
        return false;
    }
    return true;
}

// The operator behind `op`, if it has a multi-RHS path and is initialised. Host state only (no HIP call).
bool usable_operator(const SpmvOperator* op, MultiOperand* out) {
    if (op == nullptr) return fail("null operator");
    *out = multi_operand_of(op);
    if (!out->has_multi) {
        fprintf(stderr, "[multi-rhs] operator '%s' has no multi-RHS path (stencil5-csr and cusparse-csr have one)\n",
                op->name ? op->name : "?");
        return false;
    }
    if (!out->ready) {
        fprintf(stderr, "[multi-rhs] operator '%s' used before init\n", op->name);
        return false;
    }
    return true;
}

}  // namespace

namespace spmv_amd {
void release_cg_multi_workspace_locked() { g_multi.release(); }

size_t cg_multi_workspace_bytes_locked() {
    const MultiWorkspace& w = g_multi;
    if (w.X == nullptr) return 0;
    return (4 * (size_t)w.n * w.k + (size_t)w.k * w.partial_cap + (size_t)w.k * slices_for(w.partial_cap) + (size_t)w.k * w.hist_cap) *
               sizeof(double) +
           (size_t)w.k * sizeof(MultiColumn);
}
}  // namespace spmv_amd

extern "C" int spmv_amd_spmm_device(const char* mode, int nrhs, const double* d_X, double* d_Y) {
    if (mode == nullptr || !check_rhs(nrhs)) return 1;
    if (d_X == nullptr || d_Y == nullptr) return fail("null block vector"), 1;
    if ((((uintptr_t)d_X | (uintptr_t)d_Y) & 7) != 0) return fail("block vectors must be 8-byte aligned"), 1;
    SpmvOperator* op = get_operator(mode);
    if (op == nullptr) {
        fprintf(stderr, "[multi-rhs] unknown operator '%s'\n", mode);
        return 1;
    }
    MultiOperand o;
    if (!usable_operator(op, &o)) return 1;
    launch_spmm(o.plan, nrhs, d_X, d_Y, nullptr, kStream);
    HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" const char* spmv_amd_spmm_variant(const char* mode) {
    SpmvOperator* op = get_operator(mode);
    if (op == nullptr) return "unknown-operator";
    const MultiOperand o = multi_operand_of(op);
    if (!o.has_multi) return "none";
    return o.ready ? o.plan.name : "uninitialised";
}

namespace {
int move_block(int nrhs, size_t n, const double* src, double* dst, bool to_device) {
    if (!check_rhs(nrhs)) return 1;
    if (src == nullptr || dst == nullptr) return fail("null block vector"), 1;
    if (n == 0) return 0;
    double* staging = device_try_alloc<double>(n * nrhs);
    if (staging == nullptr) return fail("no device memory for the staging copy"), 1;
    if (to_device) {
        upload(staging, src, n * nrhs);
        launch_interleave(nrhs, n, staging, dst, kStream);
    } else {
        HIP_CHECK(hipStreamSynchronize(kStream));
        launch_deinterleave(nrhs, n, src, staging, kStream);
        HIP_CHECK(hipStreamSynchronize(kStream));
        download(dst, staging, n * nrhs);
    }
    HIP_CHECK(hipStreamSynchronize(kStream));
    device_release(staging);
    return 0;
}
}  // namespace

extern "C" int spmv_amd_block_to_device(int nrhs, size_t n, const double* host_columns, double* d_X) {
    return move_block(nrhs, n, host_columns, d_X, true);
}

extern "C" int spmv_amd_block_to_host(int nrhs, size_t n, const double* d_X, double* host_columns) {
    return move_block(nrhs, n, d_X, host_columns, false);
}

extern "C" int spmv_amd_cg_solve_device_multi(SpmvOperator* op, MatrixData* mat, int nrhs, const double* B, double* X,
                                              const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (!check_rhs(nrhs)) return 1;
    if (mat == nullptr || B == nullptr || X == nullptr || config == nullptr || stats == nullptr)
        return fail("null argument"), 1;
    MultiOperand o;
    if (!usable_operator(op, &o)) return 1;
    if (o.plan.rows != o.plan.cols || mat->rows != o.plan.rows) {
        fprintf(stderr, "[CG-MULTI] the operator holds a %d x %d matrix, mat->rows = %d: a square system of that size is required\n",
                o.plan.rows, o.plan.cols, mat->rows);
        return 1;
    }
    if (config->max_iters < 0) return fail("max_iters < 0"), 1;
    const int n = mat->rows, k = nrhs;
    const CGConfig cfg = *config;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const long long vec_count = ((long long)n + kBlock - 1) / kBlock;
    const long long spmm_count = o.plan.blocks;
    const long long partial_cap = vec_count > spmm_count ? vec_count : spmm_count;
    if (!ensure_workspace(n, k, device, partial_cap, cfg.max_iters + 1)) return 1;
    MultiWorkspace& w = g_multi;

    // B and x0 arrive as k columns one after the other: through AP (free until the first SpMM) into interleaved R and X
    upload(w.AP, B, (size_t)n * k);
    launch_interleave(k, (size_t)n, w.AP, w.R, kStream);
    HIP_CHECK(hipStreamSynchronize(kStream));
    upload(w.AP, X, (size_t)n * k);
    launch_interleave(k, (size_t)n, w.AP, w.X, kStream);
    HIP_CHECK(hipStreamSynchronize(kStream));

    std::vector<MultiColumn> h_cols((size_t)k);
    StageTimers T(cfg.enable_detailed_timers != 0, kStream);
    auto reduce = [&](long long count, int which) {
        launch_reduce(k, w.partials, count, w.slices, which, cfg.tolerance, w.cols, w.hist, w.hist_cap);
    };
    auto read_columns = [&] { download(h_cols.data(), w.cols, (size_t)k); };

    T.total.begin(kStream);
    T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, w.X, w.AP, nullptr, kStream); });
    T.run(&T.t_blas, [&] { launch_vector_step(k, 0, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
    T.run(&T.t_red, [&] { reduce(vec_count, 0); });
    read_columns();
    if (cfg.verbose >= 1)
        for (int j = 0; j < k; ++j) printf("[CG-MULTI %d] Initial residual: %e\n", j, h_cols[j].b_norm);
    for (int it = 0; it < cfg.max_iters; ++it) {
        bool any = false;
        for (int j = 0; j < k; ++j) any = any || !h_cols[j].done;
        if (!any) break;
        T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, w.P, w.AP, w.partials, kStream); });
        T.run(&T.t_red, [&] { reduce(spmm_count, 1); });
        T.run(&T.t_blas, [&] { launch_vector_step(k, 1, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
        T.run(&T.t_red, [&] { reduce(vec_count, 2); });
        T.run(&T.t_blas, [&] { launch_vector_step(k, 2, n, w.cols, w.X, w.R, w.P, w.AP, w.partials, vec_count); });
        read_columns();  // synchronises: the stopping test of every column
        if (cfg.verbose >= 2)
            for (int j = 0; j < k; ++j)
                if (h_cols[j].active)
                    printf("[CG-MULTI %d] Iter %3d: residual = %e (rel = %e)\n", j, h_cols[j].iterations, h_cols[j].residual,
                           h_cols[j].residual / h_cols[j].b_norm);
    }
    T.total.end(kStream);
    const double total_ms = T.total.elapsed_ms();
    HIP_CHECK(hipGetLastError());

    // the solution back as k columns one after the other (outside the timed region, as the upload)
    launch_deinterleave(k, (size_t)n, w.X, w.AP, kStream);
    HIP_CHECK(hipStreamSynchronize(kStream));
    download(X, w.AP, (size_t)n * k);
    // each column's recorded history only (the buffer may be longer: it keeps the largest max_iters seen)
    g_multi_history.assign((size_t)k, std::vector<double>());
    for (int j = 0; j < k; ++j) {
        const MultiColumn& c = h_cols[j];
        const int count = c.iterations + 1 < w.hist_cap ? c.iterations + 1 : w.hist_cap;
        g_multi_history[j].resize((size_t)count);
        download(g_multi_history[j].data(), w.hist + (size_t)j * w.hist_cap, (size_t)count);
        CGStats& st = stats[j];
        fill_device_stats(&st, c.iterations, c.done != 0, c.residual, c.b_norm, cfg, total_ms, T.t_spmv, T.t_blas, T.t_red);
        solution_checksums(X + (size_t)j * n, n, &st.solution_sum, &st.solution_norm);
        if (cfg.verbose >= 1) {
            printf("[CG-MULTI %d] Converged: %s\n", j, st.converged ? "YES" : "NO");
            printf("[CG-MULTI %d] Iterations: %d\n", j, st.iterations);
            printf("[CG-MULTI %d] Final residual: %e\n", j, st.residual_norm);
        }
    }
    if (cfg.verbose >= 1) {
        printf("[CG-MULTI] %d systems, time breakdown (whole batch):\n", k);
        printf("     Total:      %.3f ms\n", total_ms);
        printf("     SpMV:       %.3f ms\n", T.t_spmv);
        printf("     BLAS1:      %.3f ms\n", T.t_blas);
        printf("     Reductions: %.3f ms\n", T.t_red);
    }
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

namespace {
bool stage_fail(const char* stage, const char* what) {
    fprintf(stderr, "[CG-MULTI] stage '%s': %s: refused\n", stage ? stage : "(null)", what);
    return false;
}
// a pointer the stage needs, aligned to `align` bytes (16: a block vector the vector kernels access in 16-byte pairs)
bool stage_pointer(const char* stage, const char* name, const void* p, int align) {
    char what[64];
    if (p == nullptr) {
        snprintf(what, sizeof what, "%s is null", name);
        return stage_fail(stage, what);
    }
    if (((uintptr_t)p & (uintptr_t)(align - 1)) != 0) {
        snprintf(what, sizeof what, "%s is not %d-byte aligned", name, align);
        return stage_fail(stage, what);
    }
    return true;
}
}  // namespace

extern "C" int spmv_amd_cg_multi_stage(const char* stage, int k, SpmvAmdCgMultiStageArgs* a) {
    // argument checks: all before the first HIP call
    enum { kSpmm, kInit, kUpdateR, kUpdateXp, kReduce } st;
    if (stage == nullptr) return stage_fail(stage, "no stage named (spmm, init, update_r, update_xp, reduce)"), 1;
    if (!strcmp(stage, "spmm")) st = kSpmm;
    else if (!strcmp(stage, "init")) st = kInit;
    else if (!strcmp(stage, "update_r")) st = kUpdateR;
    else if (!strcmp(stage, "update_xp")) st = kUpdateXp;
    else if (!strcmp(stage, "reduce")) st = kReduce;
    else return stage_fail(stage, "unknown stage (spmm, init, update_r, update_xp, reduce)"), 1;
    if (k < 1 || k > kMaxRhs) return stage_fail(stage, "k is not 1 to 8"), 1;
    if (a == nullptr) return stage_fail(stage, "null arguments"), 1;
    MultiOperand o;
    if (st == kSpmm) {
        if (!stage_pointer(stage, "X", a->X, 8) || !stage_pointer(stage, "AP", a->AP, 8)) return 1;
        if (a->partials != nullptr && !stage_pointer(stage, "partials", a->partials, 8)) return 1;
        if (a->xcd_run < 0) return stage_fail(stage, "xcd_run < 0"), 1;
        if (a->mode == nullptr) return stage_fail(stage, "no operator named"), 1;
        SpmvOperator* op = get_operator(a->mode);
        if (op == nullptr) return stage_fail(stage, "unknown operator"), 1;
        if (!usable_operator(op, &o)) return stage_fail(stage, "the operator has no usable multi-RHS path"), 1;
    } else if (st == kReduce) {
        if (a->count < 1) return stage_fail(stage, "count < 1"), 1;
        if (a->which < 0 || a->which > 2) return stage_fail(stage, "which is not 0, 1 or 2"), 1;
        if (a->hist_cap < 0) return stage_fail(stage, "hist_cap < 0"), 1;
        if (a->which == 0 && a->hist_cap < 1) return stage_fail(stage, "hist_cap < 1 for step 0, which writes the first entry"), 1;
        if (!stage_pointer(stage, "partials", a->partials, 8) || !stage_pointer(stage, "cols", a->cols, 8)) return 1;
        if (a->hist_cap > 0 && !stage_pointer(stage, "hist", a->hist, 8)) return 1;
    } else {
        if (a->n < 1 || a->n > (size_t)INT_MAX) return stage_fail(stage, "n < 1 or beyond the solver's int rows"), 1;
        if (st != kInit && !stage_pointer(stage, "cols", a->cols, 8)) return 1;
        if (st != kUpdateXp && (!stage_pointer(stage, "AP", a->AP, 16) || !stage_pointer(stage, "partials", a->partials, 8))) return 1;
        if (!stage_pointer(stage, "R", a->R, 16)) return 1;
        if (st != kUpdateR && !stage_pointer(stage, "P", a->P, 16)) return 1;
        if (st == kUpdateXp && !stage_pointer(stage, "X", a->X, 16)) return 1;
    }

    MultiColumn* cols = reinterpret_cast<MultiColumn*>(a->cols);
    double* slices = nullptr;
    if (st == kSpmm) {
        SpmmPlan plan = o.plan;
        if (a->xcd_run > 0) plan.xcd_run = a->xcd_run;
        launch_spmm(plan, k, a->X, a->AP, a->partials, kStream);
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
