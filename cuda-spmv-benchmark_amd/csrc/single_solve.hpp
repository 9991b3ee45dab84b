// single_solve.hpp -- the host side the single-vector preconditioned solvers share around their loops (pcg.hip: preconditioned CG;
// bicgstab.hip: BiCGSTAB; gcr.hip: GCR(m)), the counterpart of multi_solve.hpp and like it built on solve_common.hpp: the argument
// checks of a solve entry point in two halves (a solver's own refusals lie between them), the product through the operator's vtable,
// the way out (solution and history back; statistics, checksums and the verbose print-out) and the launch of a streaming kernel
// template by kind. Host code only: no kernel lives here (the reduction the three share is reduce_device.hpp's
// sum_values_last_block). Every function that prints takes the tag it prints under ("PCG", "BICGSTAB", "GCR"): each solver keeps its
// sentences. The loops, their launch order, the kernels, the scalar records, the workspaces and what a solver does once run_device has
// refused stay each solver's own: these are pieces a solver calls where it needs them, not one prologue or epilogue for all three.
#pragma once

#include <stdio.h>

#include <vector>

#include "device_runtime.hpp"
#include "precond.hpp"
#include "solve_common.hpp"

namespace spmv_amd {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators
constexpr int kWave = 64;                 // the streaming kernels: one wavefront per workgroup, one 16-byte pair per lane

// kernel<kJac>(n, ...) on stream_grid(n) one-wave workgroups, kJac chosen by `jac`; `count` (the grid, as the kernels that write two
// values side by side take it) may be named among the arguments.
#define SPMV_AMD_STREAM_LAUNCH(kernel, jac, n, ...)                                               \
    do {                                                                                          \
        const dim3 grid(stream_grid(n)), block(kWave);                                            \
        const int count = (int)grid.x;                                                            \
        (void)count;                                                                              \
        if (jac) hipLaunchKernelGGL(kernel<true>, grid, block, 0, kStream, n, __VA_ARGS__);       \
        else hipLaunchKernelGGL(kernel<false>, grid, block, 0, kStream, n, __VA_ARGS__);          \
    } while (0)

// ---- argument checks: host state only, all before the first HIP call. False: refused, said on stderr behind [tag] ----
// The first half: null arguments, an operator without the device-native interface, max_iters < 0.
inline bool check_solve_arguments(const char* tag, const SpmvOperator* op, const MatrixData* mat, const SpmvAmdPrecond* m, const double* b,
                                  const double* x, const CGConfig* config, const CGStats* stats) {
    if (op == nullptr || mat == nullptr || m == nullptr || b == nullptr || x == nullptr || config == nullptr || stats == nullptr) {
        fprintf(stderr, "[%s] null argument\n", tag);
        return false;
    }
    if (op->run_device == nullptr) {
        fprintf(stderr, "[%s] operator '%s' does not support the device-native interface\n", tag, op->name ? op->name : "?");
        return false;
    }
    if (config->max_iters < 0) {
        fprintf(stderr, "[%s] max_iters < 0\n", tag);
        return false;
    }
    return true;
}

// The second half: one of this library's operators is initialised and holds the square matrix of mat->rows rows; mat->rows >= 1; the
// preconditioner is for that many rows and belongs to the operator (precond_matches, which speaks behind [PCG] for every solver).
inline bool check_solve_system(const char* tag, const SpmvOperator* op, const MatrixData* mat, const SpmvAmdPrecond* m) {
    const DiagonalSource d = diagonal_source_of(op);
    if (d.owner != nullptr) {
        if (!d.ready) {
            fprintf(stderr, "[%s] operator '%s' used before init\n", tag, op->name);
            return false;
        }
        if (d.rows != d.cols || mat->rows != d.rows) {
            fprintf(stderr, "[%s] the operator holds a %d x %d matrix, mat->rows = %d: a square system of that size is required\n", tag, d.rows,
                    d.cols, mat->rows);
            return false;
        }
    }
    if (mat->rows < 1) {
        fprintf(stderr, "[%s] mat->rows < 1\n", tag);
        return false;
    }
    if (m->n != mat->rows) {
        fprintf(stderr, "[%s] the preconditioner is for %d rows, mat->rows = %d\n", tag, m->n, mat->rows);
        return false;
    }
    return precond_matches(op, m, d);
}

// ---- the product: out = A in through the vtable. A refusal is said once and raises `failed`; what follows it is the solver's ----
inline void operator_product(const char* tag, const SpmvOperator* op, const double* in, double* out, bool& failed) {
    if (op->run_device(in, out) != 0) {
        fprintf(stderr, "[%s] operator '%s': run_device failed\n", tag, op->name);
        failed = true;
    }
}
inline void timed_product(const char* tag, const SpmvOperator* op, StageTimers& T, const double* in, double* out, bool& failed) {
    T.run(&T.t_spmv, [&] { operator_product(tag, op, in, out, failed); });
}

// ---- the way out (outside the timed region, as the upload) ----
// The solution and the recorded history back: min(iterations + 1, hist_cap) entries (the buffer keeps the largest max_iters seen).
inline void download_solution(double* x, const double* d_x, int n, int iterations, const double* d_hist, int hist_cap,
                              std::vector<double>& history) {
    download(x, d_x, (size_t)n);
    const int entries = iterations + 1 < hist_cap ? iterations + 1 : hist_cap;
    history.assign((size_t)entries, 0.0);
    download(history.data(), d_hist, (size_t)entries);
}

// What the host needs of a solver's scalar record once the loop has ended.
struct SolveSummary {
    int iterations;
    bool converged;         // stopping test met
    double residual, b_norm;
    const char* breakdown;  // null: none; else the scalar the breakdown line names ("pAp or r.z", "sigma = r^.v", ...)
};

// Statistics and checksums of the downloaded solution and, under verbose >= 1, the verdict and the time breakdown behind [tag-DEVICE].
inline void report_solve(const char* tag, const SolveSummary& s, const double* x, int n, const CGConfig& cfg, const StageTimers& T,
                         double total_ms, CGStats* stats) {
    fill_device_stats(stats, s.iterations, s.converged, s.residual, s.b_norm, cfg, total_ms, T.t_spmv, T.t_blas, T.t_red);
    solution_checksums(x, n, &stats->solution_sum, &stats->solution_norm);
    if (cfg.verbose < 1) return;
    if (s.breakdown != nullptr) printf("[%s-DEVICE] Breakdown in iteration %d (%s zero or not finite)\n", tag, s.iterations, s.breakdown);
    printf("[%s-DEVICE] Converged: %s\n", tag, stats->converged ? "YES" : "NO");
    printf("[%s-DEVICE] Iterations: %d\n", tag, stats->iterations);
    printf("[%s-DEVICE] Final residual: %e\n", tag, stats->residual_norm);
    printf("[%s-DEVICE] Time breakdown:\n", tag);
    printf("     Total:      %.3f ms\n", stats->time_total_ms);
    printf("     SpMV:       %.3f ms\n", stats->time_spmv_ms);
    printf("     BLAS1:      %.3f ms\n", stats->time_blas1_ms);
    printf("     Reductions: %.3f ms\n", stats->time_reductions_ms);
}

}  // namespace spmv_amd
