// multi_solve.hpp -- the host side the batched solvers share around their loops (cg_multi.hip: CG; pcg_multi.hip: preconditioned
// CG; bicgstab_multi.hip: BiCGSTAB): the workspace, the argument checks, the way in (upload, interleave) and the way out (de-interleave, download, histories,
// statistics, print-out), the per-iteration read of the column records and the choice of a kernel template's instance by k. Host code
// only: no kernel lives here, so spmm_kernels.hip (the operand entry points) includes it too. Every function that prints takes the tag it prints under ("CG-MULTI", "PCG-MULTI", "BICGSTAB-MULTI"): each
// solver keeps its sentences. The loops, their launch order, the kernels and the column records stay each solver's own.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "solve_common.hpp"

namespace spmv_amd {

constexpr hipStream_t kBatchStream = nullptr;  // default stream, shared with the operators

inline bool batched_fail(const char* tag, const char* what) {
    fprintf(stderr, "[%s] %s\n", tag, what);
    return false;
}

// f(std::integral_constant<int, K>) for k = K in 1..8; false, and nothing is called, for any other k.
template <class F>
bool dispatch_k(int k, F&& f) {
    switch (k) {
        case 1: f(std::integral_constant<int, 1>{}); return true;
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 3: f(std::integral_constant<int, 3>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
        case 5: f(std::integral_constant<int, 5>{}); return true;
        case 6: f(std::integral_constant<int, 6>{}); return true;
        case 7: f(std::integral_constant<int, 7>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        default: return false;
    }
}

// ---- argument checks: host state only, all before the first HIP call ----
inline bool check_rhs(const char* tag, int nrhs) {
    if (nrhs < 1 || nrhs > kMaxRhs) {
        fprintf(stderr, "[%s] nrhs = %d: 1 to %d right-hand sides are supported\n", tag, nrhs, kMaxRhs);
        return false;
    }
    return true;
}

// The operator behind `op` (not null), if it has a multi-RHS path and is initialised.
inline bool usable_operator(const char* tag, const SpmvOperator* op, MultiOperand* out) {
    *out = multi_operand_of(op);
    if (!out->has_multi) {
        fprintf(stderr, "[%s] operator '%s' has no multi-RHS path (stencil5-csr, stencil7-csr and cusparse-csr have one)\n", tag,
                op->name ? op->name : "?");
        return false;
    }
    if (!out->ready) {
        fprintf(stderr, "[%s] operator '%s' used before init\n", tag, op->name);
        return false;
    }
    return true;
}

// What both batched entry points require of their arguments. operand_tag: the tag of the refusals about nrhs and the operator
// ("multi-rhs" where the entry point shares them with the operand entry points of spmm_kernels.hip).
inline bool check_batched_system(const char* tag, const char* operand_tag, const SpmvOperator* op, const MatrixData* mat, int nrhs,
                                 const double* B, const double* X, const CGConfig* config, const CGStats* stats, MultiOperand* operand) {
    if (!check_rhs(operand_tag, nrhs)) return false;
    if (mat == nullptr || B == nullptr || X == nullptr || config == nullptr || stats == nullptr) return batched_fail(tag, "null argument");
    if (op == nullptr) return batched_fail(tag, "null operator");
    if (config->max_iters < 0) return batched_fail(tag, "max_iters < 0");
    if (!usable_operator(operand_tag, op, operand)) return false;
    if (operand->plan.rows != operand->plan.cols || mat->rows != operand->plan.rows) {
        fprintf(stderr, "[%s] the operator holds a %d x %d matrix, mat->rows = %d: a square system of that size is required\n", tag,
                operand->plan.rows, operand->plan.cols, mat->rows);
        return false;
    }
    return true;
}

// ---- workspace: kept between calls (like the other CG solvers'), released with them ----
template <class Column>
struct BatchedWorkspace {
    const int values;  // dot-product values per launch: 1 (CG), 2 (preconditioned CG: r.r and r.z)
    int n = 0, k = 0, device = -1;
    double *X = nullptr, *R = nullptr, *P = nullptr, *AP = nullptr;
    double *D = nullptr, *Z = nullptr;  // kind "chebyshev" only: they join with its first solve
    double* partials = nullptr;         // values x k x max(SpMM partials, vector partials)
    double* slices = nullptr;           // values x k x slices of that
    Column* cols = nullptr;
    double* hist = nullptr;  // k x hist_cap
    int hist_cap = 0;
    long long partial_cap = 0;  // per value and column

    explicit BatchedWorkspace(int values_) : values(values_) {}

    void release() {
        device_release(X);
        device_release(R);
        device_release(P);
        device_release(AP);
        device_release(D);
        device_release(Z);
        device_release(partials);
        device_release(slices);
        device_release(cols);
        device_release(hist);
        n = k = 0, device = -1, hist_cap = 0, partial_cap = 0;
    }

    // Device bytes held now (0: none).
    size_t bytes() const {
        if (X == nullptr) return 0;
        return ((D != nullptr ? 6 : 4) * (size_t)n * k + values * (size_t)k * partial_cap + values * (size_t)k * slices_for(partial_cap) +
                (size_t)k * hist_cap) *
                   sizeof(double) +
               (size_t)k * sizeof(Column);
    }

    // Allocates the workspace for (n, k, partial slots) if it is not there already, D and Z when with_dz asks for them, and the
    // history (each request sized against the free memory first).
    bool ensure(const char* tag, int n_, int k_, int device_, long long partial_cap_, int hist_cap_, bool with_dz) {
        if (X != nullptr && (n != n_ || k != k_ || device != device_ || partial_cap < partial_cap_)) release();
        const size_t count = (size_t)n_ * k_, vec = count * sizeof(double);
        char what[64];
        snprintf(what, sizeof what, "%d systems of %d rows%s", k_, n_, with_dz ? " (chebyshev)" : "");
        if (X == nullptr) {
            const size_t need = (with_dz ? 6 : 4) * vec + values * (size_t)k_ * partial_cap_ * sizeof(double) +
                                values * (size_t)k_ * slices_for(partial_cap_) * sizeof(double) + (size_t)k_ * hist_cap_ * sizeof(double) +
                                ((size_t)64 << 20);
            if (!device_has_room(need, tag, what)) return false;
            X = device_try_alloc<double>(count);
            R = device_try_alloc<double>(count);
            P = device_try_alloc<double>(count);
            AP = device_try_alloc<double>(count);
            partials = device_try_alloc<double>(values * (size_t)k_ * partial_cap_);
            slices = device_try_alloc<double>(values * (size_t)k_ * slices_for(partial_cap_));
            cols = device_try_alloc<Column>((size_t)k_);
            if (!X || !R || !P || !AP || !partials || !slices || !cols) {
                release();
                return batched_fail(tag, "the workspace could not be allocated: refused");
            }
            n = n_, k = k_, device = device_, partial_cap = partial_cap_;
        }
        if (with_dz && D == nullptr) {
            if (!device_has_room(2 * vec + ((size_t)64 << 20), tag, what)) return false;
            D = device_try_alloc<double>(count);
            Z = device_try_alloc<double>(count);
            if (!D || !Z) {
                device_release(D);
                device_release(Z);
                return batched_fail(tag, "the Chebyshev block vectors could not be allocated: refused");
            }
        }
        if (!grow_history(hist, hist_cap, hist_cap_, (size_t)k_)) return batched_fail(tag, "the history could not be allocated: refused");
        return true;
    }
};

// ---- the way in ----
// B and x0 arrive as k columns one after the other: through AP (free until the first SpMM) into interleaved R and X.
// clear_columns: the column records start as zeros (a loop whose kernels read a record before its first scalar step).
template <class Column>
void load_block_system(BatchedWorkspace<Column>& w, int k, int n, const double* B, const double* X, bool clear_columns = false) {
    upload(w.AP, B, (size_t)n * k);
    launch_interleave(k, (size_t)n, w.AP, w.R, kBatchStream);
    HIP_CHECK(hipStreamSynchronize(kBatchStream));
    upload(w.AP, X, (size_t)n * k);
    launch_interleave(k, (size_t)n, w.AP, w.X, kBatchStream);
    if (clear_columns) HIP_CHECK(hipMemsetAsync(w.cols, 0, (size_t)k * sizeof(Column), kBatchStream));
    HIP_CHECK(hipStreamSynchronize(kBatchStream));
}

// ---- the column records as the host side needs them: each solver fills this from its own record ----
struct ColumnSummary {
    int iterations;
    bool converged;  // stopping test met
    bool breakdown;  // stopped without it (not batched CG)
    double residual, b_norm;
    bool active;  // took part in the last iteration
    const char* breakdown_scalar = nullptr;  // what the breakdown line names (null: CG's "pAp or r.z")
};

// One small blocking read of the k column records: the stopping test of every column.
template <class Column, class Summarise>
void read_columns(const BatchedWorkspace<Column>& w, int k, Summarise&& summarise, std::vector<ColumnSummary>& out) {
    Column h[kMaxRhs];
    download(h, w.cols, (size_t)k);
    out.resize((size_t)k);
    for (int j = 0; j < k; ++j) out[(size_t)j] = summarise(h[j]);
}

inline bool any_column_running(const std::vector<ColumnSummary>& cols) {
    bool any = false;
    for (const ColumnSummary& c : cols) any = any || !(c.converged || c.breakdown);
    return any;
}

// verbose >= 1. precond_kind: named on the line (null: no preconditioner to name).
inline void print_initial_residuals(const char* tag, const std::vector<ColumnSummary>& cols, const char* precond_kind) {
    for (size_t j = 0; j < cols.size(); ++j) {
        if (precond_kind != nullptr) printf("[%s %d] Initial residual: %e (preconditioner %s)\n", tag, (int)j, cols[j].b_norm, precond_kind);
        else printf("[%s %d] Initial residual: %e\n", tag, (int)j, cols[j].b_norm);
    }
}

// verbose >= 2: one line per column that took part in the iteration just read.
inline void print_iteration(const char* tag, const std::vector<ColumnSummary>& cols) {
    for (size_t j = 0; j < cols.size(); ++j)
        if (cols[j].active)
            printf("[%s %d] Iter %3d: residual = %e (rel = %e)\n", tag, (int)j, cols[j].iterations, cols[j].residual,
                   cols[j].residual / cols[j].b_norm);
}

// ---- the way out (outside the timed region, as the upload) ----
// The solution back as k columns one after the other, each column's recorded history into history_out (the buffer may be longer: it
// keeps the largest max_iters seen), its statistics and checksums, and under verbose >= 1 the verdicts and the time breakdown.
template <class Column>
void finish_batched_solve(const char* tag, BatchedWorkspace<Column>& w, int k, int n, double* X, CGStats* stats, const CGConfig& cfg,
                          const StageTimers& T, double total_ms, const std::vector<ColumnSummary>& cols,
                          std::vector<std::vector<double>>& history_out) {
    HIP_CHECK(hipGetLastError());
    launch_deinterleave(k, (size_t)n, w.X, w.AP, kBatchStream);
    HIP_CHECK(hipStreamSynchronize(kBatchStream));
    download(X, w.AP, (size_t)n * k);
    history_out.assign((size_t)k, std::vector<double>());
    for (int j = 0; j < k; ++j) {
        const ColumnSummary& c = cols[(size_t)j];
        const int count = c.iterations + 1 < w.hist_cap ? c.iterations + 1 : w.hist_cap;
        history_out[(size_t)j].resize((size_t)count);
        download(history_out[(size_t)j].data(), w.hist + (size_t)j * w.hist_cap, (size_t)count);
        CGStats& st = stats[j];
        fill_device_stats(&st, c.iterations, c.converged, c.residual, c.b_norm, cfg, total_ms, T.t_spmv, T.t_blas, T.t_red);
        solution_checksums(X + (size_t)j * n, n, &st.solution_sum, &st.solution_norm);
        if (cfg.verbose >= 1) {
            if (c.breakdown)
                printf("[%s %d] Breakdown in iteration %d (%s zero or not finite)\n", tag, j, c.iterations,
                       c.breakdown_scalar ? c.breakdown_scalar : "pAp or r.z");
            printf("[%s %d] Converged: %s\n", tag, j, st.converged ? "YES" : "NO");
            printf("[%s %d] Iterations: %d\n", tag, j, st.iterations);
            printf("[%s %d] Final residual: %e\n", tag, j, st.residual_norm);
        }
    }
    if (cfg.verbose >= 1) {
        printf("[%s] %d systems, time breakdown (whole batch):\n", tag, k);
        printf("     Total:      %.3f ms\n", total_ms);
        printf("     SpMV:       %.3f ms\n", T.t_spmv);
        printf("     BLAS1:      %.3f ms\n", T.t_blas);
        printf("     Reductions: %.3f ms\n", T.t_red);
    }
}

}  // namespace spmv_amd
