// precond.hpp -- what pcg.hip (the preconditioned loop, kinds "none", "jacobi", "chebyshev") and multigrid.hip (kind "multigrid",
// DESIGN.md section 15) share: the preconditioner record, pcg.hip's set-up passes and Chebyshev kernels behind host launchers -- the
// multigrid smoother IS section 14's application, run by the same kernels --, and the multigrid cycle the loop calls.
#pragma once

#include "device_runtime.hpp"
#include "solve_common.hpp"

namespace spmv_amd {
struct MgHierarchy;  // multigrid.hip
}

enum PrecondKind { kNone = 0, kJacobi = 1, kChebyshev = 2, kMultigrid = 3 };
constexpr int kChebMaxDegree = 32;

struct SpmvAmdPrecond {
    int kind = kNone;
    int n = 0;
    const void* owner = nullptr;  // the operator state the diagonal came from (DiagonalSource::owner); null: a caller's diagonal
    unsigned long long generation = 0;
    double* dinv = nullptr;       // device, n values ("jacobi", "chebyshev", "multigrid": level 0's)
    int degree = 0;               // "chebyshev": steps = SpMVs per application
    double lambda_min = 0.0, lambda_max = 0.0;
    double coef[1 + 2 * kChebMaxDegree] = {0.0};  // c0, h_1, g_1, h_2, g_2, ...
    spmv_amd::MgHierarchy* mg = nullptr;          // "multigrid": the levels (owned)
};

namespace spmv_amd {

// ---- pcg.hip ----
// dinv of a CSR by the diagonal pass (d_i = the sum of row i's entries in column i, CSR order, from 0.0; dinv_i = 1.0 / d_i) with its
// validity rule. Returns the device array, or null: *bad_row >= 0 names the first offending row, -1 means no device memory (said on
// stderr; the row sentence is the caller's). Synchronises.
double* inverse_diagonal_of_csr(const SlabCsr& m, int n, int* bad_row);
// The symmetric Gershgorin bound of D^-1/2 A D^-1/2 (pcg.hip, gershgorin_kernel). Synchronises.
double gershgorin_of_csr(const SlabCsr& m, int n, const double* dinv);
// c0, h_1, g_1, ... of the degree-k Chebyshev polynomial on [lmin, lmax] (api.h states the operations).
void chebyshev_coefficients(int degree, double lmin, double lmax, double* coef);
// term 0 from a residual that is only read: u = dinv r ; d = c0 u ; z = d (cheb_term0_kernel<2>, no partials)
void launch_cheb_term0_apply(size_t n, const double* r, const double* dinv, double c0, double* d, double* z);
// one step behind a SpMV that wrote w = A z (cheb_step_kernel): d and z in place; last: the partials of r.z at partials[blk],
// stream_grid(n) of them
void launch_cheb_step(size_t n, const double* w, const double* r, const double* dinv, double g, double h, double* d, double* z, bool last,
                      double* partials);

// ---- multigrid.hip ----
void mg_destroy(MgHierarchy* h);
// One V-cycle on the hierarchy's own vectors: z = M^-1 r, r (level 0's rows, 16-byte aligned) only read. z: where the result is (a
// vector the hierarchy owns); rz_partials / rz_count: the partials of r.z the last post-smoothing update left. T (may be null): the
// solve's timers -- launches that carry a SpMV count as SpMV time, the others as BLAS1 time.
struct MgCycleResult {
    double* z = nullptr;
    const double* rz_partials = nullptr;
    int rz_count = 0;
};
MgCycleResult mg_cycle(MgHierarchy* h, const double* r, StageTimers* T);
double* mg_result_vector(MgHierarchy* h);  // a level-0 vector of the hierarchy (what a loop hands on when no cycle ran)

}  // namespace spmv_amd
