// multi_rhs.hpp -- one matrix, up to 8 right-hand sides: SpMM launchers (spmm_kernels.hip) and the records of the batched solvers
// (cg_multi.hip: CG; pcg_multi.hip: preconditioned CG; bicgstab_multi.hip: BiCGSTAB; their shared device helpers: multi_rhs_device.hpp; their shared host
// scaffold: multi_solve.hpp).
// Every launcher enqueues on the given stream and returns; none synchronises.
//
// Block vectors are row-interleaved: element (row, column j) of a block of k columns lives at X[row * k + j]. One lane reads a
// row's k values as one run of 8k bytes (16-byte loads where k is even and the pointer allows), and the solver streams 4-5
// arrays in lock step instead of 4-5 k separate vectors (lock-step streams in different 32 GiB classes cost
// 6.5 %).
//
// Column independence: column j of every kernel here is computed by exactly the instructions that compute column 0 of a
// k = 1 launch -- per-column accumulators, explicit fma(), -ffp-contract=off -- and every dot product of column j is formed
// over the same row blocks in the same order whatever k is and whatever slot j the column sits in. A column's results
// therefore depend on that column's data only (tests/test_multi_rhs_gpu.py checks this bit for bit).
#pragma once

#include "kernels.hpp"
#include "spmv_amd.h"

namespace spmv_amd {

constexpr int kMaxRhs = 8;

// Every dot product of the batched solvers is summed in two stages: slices of kReduceSlice workgroup partials first
// (multi_reduce_slices_kernel, multi_rhs_device.hpp), then the slice sums of each column.
constexpr int kReduceSlice = 256 * 16;
inline int slices_for(long long count) { return (int)((count + kReduceSlice - 1) / kReduceSlice); }

// Which kernel family one multi-RHS product of an operator takes. The stencil kinds follow the operator's single-vector
// variant (Stencil5Plan::variant), so a forced variant is honoured here too.
// Stencil7Lds: the block product of a complete 7-point level (stencil7_spmm.hip), made by plan_spmm_stencil7 only.
enum class SpmmKind { StencilLds, StencilDirect, StencilGeneric, StencilCsrLoop, Csr, Stencil7Lds };

struct SpmmPlan {
    SlabCsr m;                 // the operator's whole matrix (single GPU: row_offset 0, no halos)
    SpmmKind kind = SpmmKind::Csr;
    int rows = 0, cols = 0;
    int col_blocks = 0;        // StencilLds / StencilDirect: 256-column blocks per grid row
    int xcd_run = 1;           // StencilLds: consecutive blocks one XCD takes of every run of 8 * xcd_run
    long long blocks = 0;      // workgroups of one launch = dot-partial slots per column
    int grid3 = 0;             // Stencil7Lds: n of the n^3 grid (m.grid_size means "2-D 5-point")
    const char* name = "";     // "spmm/stencil5-row-lds", ...
};
SpmmPlan plan_spmm(const SlabCsr& m, Stencil5Variant stencil_variant, bool csr_operator, int rows, int cols);

// Y = A X for k = 1..8 interleaved columns. d_partials (may be null; square matrices): partials[j * plan.blocks + block] =
// sum over the block's rows of X[row][j] * (A X)[row][j]. X and Y must be 8-byte aligned; 16-byte aligned X and Y with an
// even k take 16-byte loads / stores.
void launch_spmm(const SpmmPlan& plan, int k, const double* X, double* Y, double* d_partials, hipStream_t stream);
// The block product of a verified complete 7-point CSR of an n^3 grid (stencil7_spmm.hip; m: a view of
// stencil7_view): "spmm/stencil7-row-lds", one wave per 128 columns of a grid row, the coefficients read once for all k columns, per
// column the bits of "spmm/csr". It forms no dot partials: launch_spmm on such a plan ignores d_partials. The level plans of the
// batched 3-D multigrid hierarchy use it; the operator's own plan on stencil7-csr stays "spmm/csr".
SpmmPlan plan_spmm_stencil7(const SlabCsr& m, int n);
void launch_stencil7_spmm(const SpmmPlan& plan, int k, const double* X, double* Y, hipStream_t stream);

// (k, n) column blocks <-> interleaved: dst[row * k + j] = src[j * n + row] and back.
void launch_interleave(int k, size_t n, const double* src_columns, double* dst_interleaved, hipStream_t stream);
void launch_deinterleave(int k, size_t n, const double* src_interleaved, double* dst_columns, hipStream_t stream);

// The multi-RHS path of one of this library's operators (operators.hip). Host-side state only: no HIP call, so the argument
// checks of the entry points built on it hold on a machine without a GPU.
struct MultiOperand {
    bool has_multi = false;  // "stencil5-csr" (and its alias "stencil5-halo-mgpu"), "stencil7-csr" and "cusparse-csr"; not the ELLPACK ones
    bool ready = false;      // initialised
    SpmmPlan plan;
};
MultiOperand multi_operand_of(const SpmvOperator* op);

// Holds the lock of the CG workspaces (cg_device.hip) for its lifetime and marks this thread as the one inside a solve: the
// batched solve obeys the same lock and the same "release asked from inside the solve" rule as cg_solve_device.
class CgWorkspaceScope {
public:
    CgWorkspaceScope();
    ~CgWorkspaceScope();
    CgWorkspaceScope(const CgWorkspaceScope&) = delete;
    CgWorkspaceScope& operator=(const CgWorkspaceScope&) = delete;
};
// Frees the batched solver's workspace (cg_multi.hip); the caller holds the workspace lock.
void release_cg_multi_workspace_locked();
// Device bytes the batched solver's workspace holds now (0: none); the caller holds the workspace lock.
size_t cg_multi_workspace_bytes_locked();

// Per-column state of a batched CG solve (device memory, one entry per column).
struct MultiColumn {
    double rr_old, pAp, alpha, beta, b_norm, residual;
    int active;      // the column takes part in the current iteration (set by the pAp step: !done)
    int done;        // converged: the column is frozen from the next iteration on
    int iterations;  // iterations this column took part in
    int pad;
};

// Per-column state of a batched preconditioned solve (pcg_multi.hip; device memory, one entry per column): pcg.hip's scalars
// of one solve, per column, with the batched loop's two flags.
struct PcgMultiColumn {
    double rz;        // r.z of the column's current residual
    double pAp, alpha, beta;
    double b_norm;    // ||r0||
    double residual;  // ||r_k||
    int active;       // the column takes part in the current iteration (set by the pAp step: !done)
    int done;         // converged or broken down: the column is frozen from the next iteration on
    int iterations;   // iterations this column took part in
    int converged;    // stopping test met
    int breakdown;    // pAp or r.z' zero or not finite: stopped, not converged
    int skip_update;  // this iteration's pAp broke down: r and x stay as they are
    int pad[2];
};
// pcg_multi.hip's Chebyshev step kernel (k = 1..8 columns, on the default stream) behind a SpMM that wrote W = A Z, for the callers
// outside that file (the batched multigrid cycle and the block application, multigrid_multi.hip): on the columns with done == 0,
// d = fma(g, dinv * fma(-1, w, r), h * d) ; z = z + d. last: the partials of r.z to partials[(k + j) * count + workgroup]; count =
// the launch's workgroups, (n + 255) / 256. Nothing is read or written once every column is done.
void launch_pcg_multi_cheb_step(int k, long long n, const PcgMultiColumn* cols, const double* W, const double* R, const double* dinv, double g,
                                double h, double* D, double* Z, int last, double* partials, long long count);
// The batched preconditioned solver's workspace (pcg_multi.hip), released and counted like the batched CG solver's; the caller
// holds the workspace lock.
void release_pcg_multi_workspace_locked();
size_t pcg_multi_workspace_bytes_locked();

// Per-column state of a batched BiCGSTAB solve (bicgstab_multi.hip; device memory, one entry per column): bicgstab.hip's scalars of
// one solve, per column, with the batched loop's two flags in the place of `stop`.
struct BicgMultiColumn {
    double rho;       // r^.r of the column's current residual
    double sigma, alpha, omega, beta;
    double b_norm;    // ||r0||
    double residual;  // the norm recorded last
    double s_norm;    // ||s|| of this iteration
    int active;       // the column takes part in the current iteration (set by the sigma step: !done)
    int done;         // converged or broken down: the column is frozen from the next iteration on
    int iterations;   // iterations this column took part in
    int converged;    // stopping test met (by the half step or by the whole one)
    int breakdown;    // 0, or which scalar stopped the column: 1 sigma, 2 omega (t.t or t.s), 3 rho'
    int x_step;       // what the x / r kernel applies to the column in this iteration: 0 nothing, 1 the half step, 2 the whole step
    int pad[2];
};
// The batched BiCGSTAB solver's workspace (bicgstab_multi.hip), released and counted like the other batched solvers'; the caller
// holds the workspace lock.
void release_bicgstab_multi_workspace_locked();
size_t bicgstab_multi_workspace_bytes_locked();

// Per-column state of a batched GCR(m) solve (gcr_multi.hip; device memory, one entry per column): gcr.hip's scalars of one solve,
// per column, with the batched loop's two flags in the place of `stop`. Beside the k records the solve keeps k PcgMultiColumn records
// whose `done` every scalar step writes with this one's: the block applications (mg_cycle_multi, launch_pcg_multi_cheb_step,
// launch_mg_multi_term0) read that field of those records and no other.
constexpr int kGcrMultiMaxRestart = 32;
struct GcrMultiColumn {
    double gamma[kGcrMultiMaxRestart];  // q.q of the basis slots filled since the last restart
    double beta[kGcrMultiMaxRestart];   // this iteration's (q.Q_i) / gamma_i, i < slot
    double alpha, rho;                  // this iteration's step length and r.q
    double b_norm;                      // ||r0||
    double residual;                    // the norm recorded last
    int done;        // converged or broken down: the column is frozen from then on -- no launch changes a bit of this record either
    int iterations;  // iterations this column took part in
    int converged;   // stopping test met
    int breakdown;   // 0, or which scalar stopped the column: 1 gamma = q.q, 2 rho = r.q
};
// term 0 of an application on k interleaved columns (multigrid_multi.hip's mg_multi_term0_kernel): d = c0 * (dinv * r) ; z = d for
// every column once one has done == 0 (cols null: all are running). D may be null: the Jacobi product, c0 = 1.0.
void launch_mg_multi_term0(int k, long long rows, const PcgMultiColumn* cols, const double* R, const double* dinv, double c0, double* D,
                           double* Z);
// The batched GCR solver's workspace (gcr_multi.hip), released like the other batched solvers'; the caller holds the workspace lock.
void release_gcr_multi_workspace_locked();

}  // namespace spmv_amd
