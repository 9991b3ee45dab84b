// multigrid.hpp -- the host side the four multigrid sources share (DESIGN.md sections 15, 17, 19, 20): the hierarchy of kind
// "multigrid" and every launch of its cycle. multigrid.hip makes the hierarchy and runs the single-vector cycle, multigrid_multi.hip the
// batched one; multigrid3d.hip and multigrid3d_multi.hip hold the launches a 3-D level adds. pcg_multi.hip reads level 0's c0 here;
// what the PCG loops call is precond.hpp's.
#pragma once

#include <vector>

#include "precond.hpp"
#include "stencil_geometry.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

namespace spmv_amd {

constexpr int kMgCoarsestDegree = 8;  // the coarsest level's Chebyshev degree

struct PcgMultiColumn;
struct MgMulti;  // multigrid_multi.hip: the levels' block vectors and SpMM plans
// Device bytes mg_multi_create will ask for, from the levels' rows alone (the creator sizes everything against free memory first).
size_t mg_multi_bytes(const MgHierarchy* h, int max_rhs);
// Allocates them and plans every level's SpMM; null (nothing left behind, said on stderr) when the device cannot provide them.
MgMulti* mg_multi_create(const MgHierarchy* h, int max_rhs);
void mg_multi_destroy(MgMulti* mm);

// A complete 5-point CSR on an n x n grid in the caller's arrays as a view, and its structure check (synchronises; sets the view's flag).
SlabCsr mg_stencil_view(int n, const int* row_ptr, const int* col_idx, const double* values);
bool mg_verify_stencil5(SlabCsr& v);
// The same for a complete 7-point CSR on an n^3 grid (2 <= n <= 674; [D,N,W,C,E,S,U], stencil_geometry.hpp). n is passed beside the
// view everywhere: the view's grid_size stays unset, it means "2-D 5-point" to the kernels that read it.
SlabCsr stencil7_view(int n, const int* row_ptr, const int* col_idx, const double* values);
bool mg_verify_stencil7(SlabCsr& v, int n);
inline long long stencil_nnz(int n) { return n >= 2 ? stencil_gridrow_base(n, n) : 1; }

// ---- the launches: the cycles make them, and so do the LAB build's spmv_amd_mg_stage, ..._mg_multi_stage and ..._mg_multi_stage3d.
// No synchronisation. Single vectors: default stream, z and r 16-byte aligned. ----
// A_c = P^T A P on the grid nc = ceil(n / 2) (3-D: nc^3), every entry a sequential sum in the order api.h states
void launch_coarsen(const SlabCsr& fine, int nc, int* row_ptr, int* col_idx, double* values);
void launch_coarsen3d(const SlabCsr& fine, int n, int* row_ptr, int* col_idx, double* values);
// r_c = P^T (r - A z) in one launch; A z and r - A z are never stored
void launch_residual_restrict(const SlabCsr& m, const double* z, const double* r, double* rc);
void launch_residual_restrict3d(const SlabCsr& m, int n, const double* z, const double* r, double* rc);
// z = fma(2.0, e_c[agg(i)], z), z in place
void launch_prolong_correct(int n, const double* ec, double* z);
void launch_prolong_correct3d(int n, const double* ec, double* z);
// The same on block vectors of k = 1..8 row-interleaved columns, on the batch stream. cols: the device column records (null: every
// column is running); nothing is read or written once every column is done. Block vectors: 8-byte aligned, 16-byte accesses wherever
// an address allows.
void launch_residual_restrict_multi(int k, const SlabCsr& m, const PcgMultiColumn* cols, const double* z, const double* r, double* rc);
void launch_residual_restrict3d_multi(int k, const SlabCsr& m, int n, const PcgMultiColumn* cols, const double* z, const double* r, double* rc);
void launch_prolong_correct_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z);
void launch_prolong_correct3d_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z);

#ifdef SPMV_AMD_LAB
// spmv_amd_mg_multi_stage (dim 2) and spmv_amd_mg_multi_stage3d (dim 3): one body, multigrid_multi.hip
int mg_multi_stage(int dim, const char* stage, int k, SpmvAmdMgMultiStageArgs* a);
#endif

// The two launches of an AMG level (amg.hip): arbitrary aggregates given as member lists (agg_ptr: coarse_rows + 1,
// members: the fine rows of each aggregate in ascending order) and as the map agg (one aggregate per fine row).
// r_c[I] = ((t_m0 + t_m1) + ...) over I's members, t_i = fma(-1.0, s_i, r_i), s_i row i's sequential fma chain; one launch, no scratch
void launch_amg_residual_restrict(const SlabCsr& m, int coarse_rows, const int* agg_ptr, const int* members, const double* z, const double* r,
                                  double* rc);
// z = fma(2.0, e_c[agg[i]], z), z in place (16-byte aligned)
void launch_amg_prolong_correct(size_t rows, const int* agg, const double* ec, double* z);
// The same two on block vectors of k = 1..8 row-interleaved columns, on the batch stream (amg_multi.hip). cols: the
// device column records (null: every column is running); nothing is read or written once every column is done. Per column the bits of
// the two above; the matrix, the member lists and agg are read once for all k columns.
void launch_amg_residual_restrict_multi(int k, const SlabCsr& m, int coarse_rows, const int* agg_ptr, const int* members,
                                        const PcgMultiColumn* cols, const double* Z, const double* R, double* Rc);
void launch_amg_prolong_correct_multi(int k, size_t rows, const int* agg, const PcgMultiColumn* cols, const double* Ec, double* Z);
#ifdef SPMV_AMD_LAB
// spmv_amd_amg_stage (k = 0: single vectors) and spmv_amd_amg_multi_stage (k = 1..8): one body, amg.hip
int amg_stage(const char* stage, int k, SpmvAmdAmgStageArgs* a);
#endif

struct MgLevel {
    int dim = 2;          // 2: an n x n 5-point stencil; 3: an n x n x n 7-point one; 0: a general CSR (an AMG level, no grid: n stays 0)
    int n = 0, rows = 0;  // the grid and its rows
    DeviceCsr A;          // levels above 0 (level 0 reads the operator's own CSR)
    SlabCsr view;
    Stencil5Plan plan;    // dim 2
    Stencil7Plan plan7;   // dim 3
    double* dinv = nullptr;  // level 0's belongs to the SpmvAmdPrecond
    bool own_dinv = true;
    double lambda_max = 0.0;
    int degree = 0;          // Chebyshev steps of the level's smoother (the coarsest level: of its solve)
    double coef[1 + 2 * kMgCoarsestDegree] = {0.0};   // c0, h_1, g_1, ...
    double *r = nullptr, *d = nullptr, *z = nullptr;  // r: levels above 0
    double* aux = nullptr;  // a 2-D row-lds plan: z' of the fused step; every other plan: w = A z
    // dim 0: level 0 runs the operator's own run_device (op), every other level launch_csr_spmv in csr_variant; a level that is not
    // the coarsest holds its aggregates on the device
    const SpmvOperator* op = nullptr;
    CsrVariant csr_variant = CsrVariant::Auto;
    int coarse_rows = 0, max_aggregate = 0;
    int *agg = nullptr, *agg_ptr = nullptr, *members = nullptr;
    bool fused() const { return dim == 2 && plan.variant == Stencil5Variant::RowLds; }
    ChebSpmv spmv() const {  // how this level runs A z (device_runtime.hpp)
        ChebSpmv a;
        if (dim == 0) {
            if (op != nullptr) a.op = op;
            else a.view = &view, a.csr = true, a.csr_variant = csr_variant;
            return a;
        }
        a.view = &view;
        if (dim == 3) a.plan7 = &plan7;
        else a.plan = &plan, a.partials = fused() ? plan.partials : 0;
        return a;
    }
    long long nnz() const { return dim == 0 ? view.nnz_local : dim == 3 ? stencil7_nnz(n) : stencil_nnz(n); }
};

struct MgHierarchy {
    int dim = 2;  // 0: an AMG hierarchy (spmv_amd_precond_create_amg, ..._amg_multi)
    double strength = 0.0, setup_ms = 0.0;  // dim 0: theta, and the host wall time of the creation
    std::vector<MgLevel> levels;
    int smoother_degree = 0;
    double* partials = nullptr;  // the r.z partials of level 0's last update
    MgMulti* multi = nullptr;    // spmv_amd_precond_create_multigrid_multi / ..._multigrid3d_multi / ..._amg_multi; null: single vectors only
    int count() const { return (int)levels.size(); }
    void release() {
        mg_multi_destroy(multi);
        multi = nullptr;
        for (MgLevel& L : levels) {
            L.A.release();
            if (L.own_dinv) device_release(L.dinv);
            device_release(L.r);
            device_release(L.d);
            device_release(L.z);
            device_release(L.aux);
            device_release(L.agg);
            device_release(L.agg_ptr);
            device_release(L.members);
        }
        levels.clear();
        device_release(partials);
    }
};

}  // namespace spmv_amd
