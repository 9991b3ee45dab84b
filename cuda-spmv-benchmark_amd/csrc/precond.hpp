// precond.hpp -- the preconditioner record and what its users share. precond.hip owns the record: the creators with their set-up passes
// (diagonal, Gershgorin bound, Chebyshev coefficients), the runner of a Chebyshev step, spmv_amd_precond_apply_device, info and destroy.
// pcg.hip (the preconditioned loop), bicgstab.hip, gcr.hip, the batched solvers and multigrid.hip (kind "multigrid", DESIGN.md section
// 15; its hierarchy and launches: multigrid.hpp) reach those through this header -- the multigrid smoother IS section 14's application,
// run by the same function on a level's operator -- and precond.hip reaches pcg.hip's term-0 kernel and reduce launch through it.
#pragma once

#include <string.h>

#include "device_runtime.hpp"
#include "solve_common.hpp"

namespace spmv_amd {
struct MgHierarchy;  // multigrid.hpp
}

enum PrecondKind { kNone = 0, kJacobi = 1, kChebyshev = 2, kMultigrid = 3 };
constexpr int kChebMaxDegree = 32;

// The kind a caller names, or -1. An entry point that takes "none" and "jacobi" alone refuses the other two itself.
inline int kind_of(const char* kind) {
    if (kind == nullptr) return -1;
    if (!strcmp(kind, "none")) return kNone;
    if (!strcmp(kind, "jacobi")) return kJacobi;
    if (!strcmp(kind, "chebyshev")) return kChebyshev;
    if (!strcmp(kind, "multigrid")) return kMultigrid;
    return -1;
}

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

// Where an application z = M^-1 r left z and the partials of r.z (the Chebyshev runner's and the multigrid cycle's report).
struct Applied {
    double* z = nullptr;
    const double* rz_partials = nullptr;
    int rz_count = 0;
};

// One launch under a solve's timers (T null: untimed). A launch that carries a SpMV counts as SpMV time (t_spmv), every other as BLAS1.
template <class F>
void stage_run(StageTimers* T, double StageTimers::*acc, F&& launch) {
    if (T != nullptr) T->run(&(T->*acc), launch);
    else launch();
}

// ---- precond.hip ----
// dinv of a CSR by the diagonal pass (d_i = the sum of row i's entries in column i, CSR order, from 0.0; dinv_i = 1.0 / d_i) with its
// validity rule. Returns the device array, or null: a row at fault is named on stderr behind `who` ("jacobi", "multigrid: level 2")
// and, where bad_row is not null, stored there; no device memory is said too. Synchronises.
double* inverse_diagonal_of_csr(const SlabCsr& m, int n, const char* who, int* bad_row);
// The symmetric Gershgorin bound of D^-1/2 A D^-1/2 (precond.hip, gershgorin_kernel). Synchronises.
double gershgorin_of_csr(const SlabCsr& m, int n, const double* dinv);
// c0, h_1, g_1, ... of the degree-k Chebyshev polynomial on [lmin, lmax] (api.h states the operations).
void chebyshev_coefficients(int degree, double lmin, double lmax, double* coef);
// What the creators check of their (non-null) operator, in this order, before the first HIP call: not one of this library's -- or,
// stencil_dim 2 / 3, not the 2-D / 3-D stencil operator (0: any of ours) -- said as "[PCG] <label>operator '<name>' is not <not_ours>"; used before init; not square
// (left to a stencil creator's stricter test behind this). False: refused, said on stderr.
bool creation_source(const SpmvOperator* op, const char* label, const char* not_ours, int stencil_dim, DiagonalSource* d);
// What every entry point that takes (op, m) checks of the pair before any HIP call; d: the operator's storage view. False: refused,
// said on stderr behind [PCG].
bool precond_matches(const SpmvOperator* op, const SpmvAmdPrecond* m, const DiagonalSource& d);

// ---- pcg.hip: what an application on its own (spmv_amd_precond_apply_device, gcr.hip) takes from the preconditioned loop ----
// Device scalars of one preconditioned solve.
struct PcgScalars {
    double rz;        // r.z of the current residual
    double pAp, alpha, beta;
    double b_norm;    // ||r0||
    double residual;  // ||r_k||
    int iterations;
    int converged;    // stopping test met
    int breakdown;    // pAp or r.z' zero or not finite: stopped, not converged
    int skip_update;  // this iteration's pAp broke down: r and x stay as they are
};
// The device record of a Chebyshev solve: the scalars every kind keeps, then what only this kind needs. pcg_step's steps 3 to 5 are
// handed the record's first member and reach the rest through it.
struct ChebScalars {
    PcgScalars s;
    int stop;        // the iteration's verdict (converged or broken down): the steps' skip flag
    int steps_done;  // step launches that did work
};
// term 0 from a residual that is only read: u = dinv r ; d = c0 u ; z = d (cheb_term0_kernel<2>). last (term 0 is the whole
// polynomial): the partials of r.z at partials[stream_grid(n) + blk]; else no partials.
void launch_cheb_term0_apply(size_t n, const double* r, const double* dinv, double c0, double* d, double* z, bool last = false,
                             double* partials = nullptr);
// nv sums of `count` partials each and the scalar step `which` (pcg.hip has the steps; 5: rz = the sum, an application on its own)
void launch_pcg_reduce(const double* partials, int count, int nv, int which, double* stage, PcgScalars* s, double tol, double* hist,
                       int hist_cap);

// One Chebyshev application in flight on one operator or level: t = fma(-1, A z, r) ; u = dinv t ; d = fma(g, u, h d) ; z = z + d.
// cheb_step runs one step in the form `a` allows: on a row-lds plan the fused launch (z' goes to aux, then z and aux change places),
// on any other stencil plan (2-D, or the Stencil7Plan of a 3-D level) the SpMV that tests `stop` into aux and cheb_step_kernel, on a general CSR level of an AMG hierarchy launch_csr_spmv into aux and cheb_step_kernel, else run_device into aux and cheb_step_kernel.
// last: the step also writes the partials of r.z to `partials` and records them in rz_partials / rz_count. False: run_device
// refused (said on stderr). cheb_steps runs steps 1 .. degree from coef (c0, h_1, g_1, ...); report: step `degree` is a last one.
struct ChebRun {
    ChebSpmv a;
    size_t n = 0;
    const double* r = nullptr;
    const double* dinv = nullptr;
    double* d = nullptr;
    double* z = nullptr;         // where z is: moves between the two vectors of a fused step
    double* aux = nullptr;       // fused: the other z vector; else w = A z
    double* partials = nullptr;  // a.partials slots (fused) or stream_grid(n) (cheb_step_kernel)
    const int* stop = nullptr;   // device flag: nothing is read once it is set (null: no test)
    int* work_count = nullptr;   // device counter of the step launches that did work (may be null)
    StageTimers* T = nullptr;    // null: untimed
    const double* rz_partials = nullptr;
    int rz_count = 0;
};
bool cheb_step(ChebRun& c, double g, double h, bool last);
bool cheb_steps(ChebRun& c, int degree, const double* coef, bool report);
// Steps 1 .. degree of m's polynomial behind a term 0 that left d and z in c -- and, at degree 0, the r.z partials behind its r.r ones.
bool cheb_after_term0(const SpmvAmdPrecond* m, ChebRun& c);

// ---- what the PCG loops call of kind "multigrid" (multigrid.hip, multigrid_multi.hip; the hierarchy itself: multigrid.hpp) ----
void mg_destroy(MgHierarchy* h);
// One V-cycle on the hierarchy's own vectors: z = M^-1 r, r (level 0's rows, 16-byte aligned) only read. z: a vector the hierarchy
// owns; the r.z partials are the ones the last post-smoothing step left. T (may be null): the solve's timers.
Applied mg_cycle(MgHierarchy* h, const double* r, StageTimers* T);
double* mg_result_vector(MgHierarchy* h);  // a level-0 vector of the hierarchy (what a loop hands on when no cycle ran)
// The block vectors and SpMM plans of a hierarchy made by spmv_amd_precond_create_multigrid_multi, ..._multigrid3d_multi or ..._amg_multi
// (null: a single-vector hierarchy).
struct MgMulti;
MgMulti* mg_multi_of(const MgHierarchy* h);
int mg_multi_capacity(const MgMulti* mm);  // max_rhs; 0 for null
// One V-cycle on k <= max_rhs interleaved columns, on the batch stream: Z = M^-1 R. Level 0 works on the caller's vectors -- R (only
// read), D and Z holding term 0 on entry, W (scratch for A Z) -- every other level on the hierarchy's. cols: the device column records
// (every launch returns at once when no column is running; a stopped column's D, Z and level vectors are scratch). Level 0's last step
// leaves the r.z partials as value 1 of `partials` (2 k count slots), where pcg_multi.hip's step 4 reads them. T may be null.
struct PcgMultiColumn;
void mg_cycle_multi(const MgHierarchy* h, int k, const PcgMultiColumn* cols, const double* R, double* D, double* Z, double* W,
                    double* partials, long long count, StageTimers* T);

}  // namespace spmv_amd
