// solve_common.hpp -- the host side every solve entry point shares around its loop (cg_single.hip, cg_slab_solve.hip, pcg.hip,
// bicgstab.hip, gcr.hip and the batched solvers): checksums of the solution, the per-stage timers, the statistics rule of a device
// solve, the history hand-out, the two halves of a workspace request and the refusals of the LAB build's stage hooks. The loops and
// their kernels stay each solver's own. Two scaffolds are built on this header: multi_solve.hpp, what the batched solvers share beyond
// it (workspace, checks, upload, download, print-out), and single_solve.hpp, what pcg.hip, bicgstab.hip and gcr.hip share (checks,
// the product, download, print-out).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "device_runtime.hpp"

namespace spmv_amd {

// sum x and sqrt(sum x^2) of a solution on the host, added in index order (the harness reports and compares them).
inline void solution_checksums(const double* x, int n, double* sum, double* norm) {
    double s = 0.0, q = 0.0;
    for (int i = 0; i < n; i++) {
        s += x[i];
        q += x[i] * x[i];
    }
    *sum = s;
    *norm = sqrt(q);
}

// The timers of one solve: `total` around the whole loop (the caller begins and ends it), `part` around one stage at a time,
// accumulated into t_spmv / t_blas / t_red. With detail off a stage is its launch and nothing else: no event is recorded, so
// nothing blocks between the launches of an iteration.
struct StageTimers {
    EventTimer total, part;
    double t_spmv = 0.0, t_blas = 0.0, t_red = 0.0;
    bool detail;
    hipStream_t stream;
    StageTimers(bool detail_, hipStream_t stream_) : detail(detail_), stream(stream_) {}
    template <class F>
    void run(double* acc, F&& launch) {
        if (detail) part.begin(stream);
        launch();
        if (detail) {
            part.end(stream);
            *acc += part.elapsed_ms();
        }
    }
};

// The statistics of a device solve, the reference's rule (cg_solver.cu:535, :601-619): its final_residual_norm is whatever it
// last copied back -- the residual of the converging iteration when the device's test was met, else the residual of the last
// iteration under verbose >= 2 (the only case in which it copies one back per iteration), else still ||r0||. `converged` is
// then recomputed on the host from that reported value, so an unconverged solve that reports ||r0|| says 0 and one that
// reports its last residual says what the same strict test says of it.
inline void fill_device_stats(CGStats* st, int iterations, bool converged_on_device, double last_residual, double b_norm, const CGConfig& cfg,
                              double total_ms, double spmv_ms, double blas_ms, double reductions_ms) {
    st->iterations = iterations;
    st->residual_norm = converged_on_device ? last_residual : (cfg.verbose >= 2 && iterations > 0 ? last_residual : b_norm);
    st->converged = (b_norm > 0.0 && st->residual_norm / b_norm < cfg.tolerance) ? 1 : 0;
    st->time_total_ms = total_ms;
    st->time_spmv_ms = spmv_ms;
    st->time_blas1_ms = blas_ms;
    st->time_reductions_ms = reductions_ms;
}

// Copies up to `cap` entries of a residual history to `out` (null: nothing is copied) and returns the history's length.
inline int copy_history(const std::vector<double>& h, double* out, int cap) {
    const int count = (int)h.size();
    for (int i = 0; i < count && i < cap && out != nullptr; ++i) out[i] = h[(size_t)i];
    return count;
}

// A workspace request is sized against hipMemGetInfo before anything is allocated (need_bytes includes the caller's margin):
// one that does not fit is refused with a sentence, never a crash. what: "20000 rows", "4 systems of 20000 rows".
inline bool device_has_room(size_t need_bytes, const char* tag, const char* what) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need_bytes <= free_b) return true;
    fprintf(stderr, "[%s] the workspace for %s needs %.2f GB, the device has %.2f GB free: refused\n", tag, what, need_bytes / 1e9,
            free_b / 1e9);
    return false;
}

// The history buffer keeps the largest max_iters seen: `columns` x `want` doubles once `cap` < want. False (cap = 0, hist
// null) when the device cannot provide it.
inline bool grow_history(double*& hist, int& cap, int want, size_t columns = 1) {
    if (cap >= want) return true;
    device_release(hist);
    cap = 0;
    hist = device_try_alloc<double>(columns * (size_t)want);
    if (hist == nullptr) return false;
    cap = want;
    return true;
}

// ---- the LAB build's stage hooks (include/spmv_amd/lab.h): their refusals ----
inline bool stage_fail(const char* tag, const char* stage, const char* what) {
    fprintf(stderr, "[%s] stage '%s': %s: refused\n", tag, stage ? stage : "(null)", what);
    return false;
}

// A pointer the stage needs, aligned to `align` bytes (16: a vector the kernels access in 16-byte pairs; 8: doubles one at a time).
inline bool stage_pointer(const char* tag, const char* stage, const char* name, const void* p, int align) {
    char what[64];
    if (p == nullptr) {
        snprintf(what, sizeof what, "%s is null", name);
        return stage_fail(tag, stage, what);
    }
    if (((uintptr_t)p & (uintptr_t)(align - 1)) != 0) {
        snprintf(what, sizeof what, "%s is not %d-byte aligned", name, align);
        return stage_fail(tag, stage, what);
    }
    return true;
}

}  // namespace spmv_amd
