// multigrid.hip -- kind "multigrid" of the preconditioned solver (pcg.hip): a symmetric V(nu, nu) cycle on a hierarchy of 5-point
// stencils made by 2 x 2 aggregation of the stencil5-csr operator's grid (include/spmv_amd/api.h states the
// algebra down to the order of every sum).
//
// Levels: level 0 is the operator's own verified CSR on an n0 x n0 grid; level l+1 has the grid ceil(n_l / 2), aggregate (I, J) =
// the fine points (2I + a, 2J + b), a, b in {0, 1}, that exist; coarsening stops at the first grid of at most 8 (or at max_levels).
// A_c = P^T A P with P piecewise constant is again a complete 5-point CSR (coarsen_kernel), so every level runs the library's own
// stencil kernels through a Stencil5Plan of its own: launch_stencil5_cheb_step where the plan is row-lds, launch_stencil5_spmv and
// precond.hip's streaming step elsewhere. Per level: dinv by precond.hip's diagonal pass, lambda_max by its Gershgorin kernel, the smoother =
// section 14's Chebyshev application of degree nu on [lambda_max / 4, lambda_max]; the coarsest level is solved by degree 8 on
// [lambda_max / 30, lambda_max] from a zero guess.
//
// The hierarchy (MgLevel, MgHierarchy) and the declarations of every launch are multigrid.hpp's; the order of a cycle's launches is
// mg_schedule.hpp's mg_vcycle, which CycleOps here and MultiOps in multigrid_multi.hip walk.
// Cycle on level l (input r, output z):
//   pre-smooth   term 0 and nu steps of the application
//   restrict     r_c[I, J] = ((t00 + t01) + t10) + t11 over the members that exist, t = fma(-1.0, (A z)_i, r_i): ONE launch
//                (residual_restrict_kernel), A z and r - A z never stored
//   recurse      e_c = cycle(l + 1, r_c)
//   correct      z = fma(2.0, e_c[agg(i)], z)   (the Galerkin operator of 2 x 2 aggregates is twice the re-discretised one)
//   post-smooth  nu + 1 step-form updates from the guess z: the first with (g, h) = (c0, 0.0), then steps 1 .. nu
// Pre- and post-smoother are the same symmetric polynomial: M^-1 is symmetric.
//
// The same hierarchy, cycle and creator serve the 3-D operator stencil7-csr (spmv_amd_precond_create_multigrid3d, DESIGN.md section
// 17): a level carries its dimension; a 3-D level is a complete 7-point CSR made by 2 x 2 x 2 aggregation, its three launches are
// multigrid3d.hip's, and it smooths with launch_stencil7_spmv on a Stencil7Plan of its own + precond.hip's streaming step.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "mg_schedule.hpp"
#include "multi_rhs.hpp"
#include "multigrid.hpp"
#include "multigrid_device.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators and pcg.hip
constexpr int kWave = 64;
constexpr int kCoarsestGrid = 8;  // coarsening stops at the first grid of at most this
constexpr int kMaxSmoother = 8;
constexpr int kMaxLevels = 32;

bool fail(const char* what) {
    fprintf(stderr, "[PCG] multigrid: %s\n", what);
    return false;
}

// the structure check of a level's view: the complete 5-point pattern of v.grid_size (dim 2), the complete 7-point one of n^3 (dim 3)
bool verified(SlabCsr& v, int dim = 2, int n = 0) {
    int* d_mismatch = device_try_alloc<int>(1);
    if (d_mismatch == nullptr) return fail("no device memory for the structure check");
    HIP_CHECK(hipMemsetAsync(d_mismatch, 0, sizeof(int), kStream));
    if (dim == 3) launch_verify_stencil7_csr(v, n, d_mismatch, kStream);
    else launch_verify_stencil5_csr(v, d_mismatch, kStream);
    HIP_CHECK(hipGetLastError());
    int mismatch = 1;
    download(&mismatch, d_mismatch, 1);  // synchronises
    device_release(d_mismatch);
    if (dim == 2) v.verified_stencil = mismatch == 0;  // the view's flag means "2-D 5-point"
    return mismatch == 0;
}

// ---- coarsening: one thread per coarse row; set-up work ----
// Every coarse entry is a sequential sum from 0.0 with plain additions: the members are walked in the order (0,0), (0,1), (1,0), (1,1),
// each member's entries in CSR order, and an entry is added to the coarse entry of the aggregate its column lies in. N_c thus sums
// N(2I, 2J + b) over b ascending, W_c sums W(2I + a, 2J) over a ascending, E_c and S_c likewise, C_c everything that stays inside.
__global__ __launch_bounds__(256) void coarsen_kernel(SlabCsr fine, int n, int nc, int* __restrict__ row_ptr, int* __restrict__ col_idx,
                                                      double* __restrict__ values) {
    const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (row >= nc * nc) return;
    const int I = row / nc, J = row - I * nc;
    double vn = 0.0, vw = 0.0, vc = 0.0, ve = 0.0, vs = 0.0;
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 2; ++b) {
            const int i = 2 * I + a, j = 2 * J + b;
            if (i >= n || j >= n) continue;
            const int fr = i * n + j;
            for (int k = fine.row_ptr[fr]; k < fine.row_ptr[fr + 1]; ++k) {
                const int c = fine.col_idx[k];
                const int ci = c / n, cj = c - ci * n;
                const int CI = ci >> 1, CJ = cj >> 1;
                const double v = fine.values[k];
                if (CI == I && CJ == J) vc = vc + v;
                else if (CI < I) vn = vn + v;
                else if (CI > I) vs = vs + v;
                else if (CJ < J) vw = vw + v;
                else ve = ve + v;
            }
        }
    }
    int at = (int)stencil_row_start(I, J, nc);
    row_ptr[row] = at;
    if (I > 0) col_idx[at] = row - nc, values[at] = vn, ++at;
    if (J > 0) col_idx[at] = row - 1, values[at] = vw, ++at;
    col_idx[at] = row, values[at] = vc, ++at;
    if (J < nc - 1) col_idx[at] = row + 1, values[at] = ve, ++at;
    if (I < nc - 1) col_idx[at] = row + nc, values[at] = vs, ++at;
    if (row == nc * nc - 1) row_ptr[nc * nc] = at;
}

// ---- residual + restriction in one launch ----
// One wave takes 128 fine columns x the 2 fine grid rows of coarse grid row I: 64 coarse values, lane l owns aggregate column l of the
// tile (fine columns ja = j0 + 2 l and jb = ja + 1). A pair of rows inside the grid (2I >= 1, 2I + 1 <= n - 2) takes the fast path:
//   * the two rows' coefficients -- 640 consecutive CSR values each, 40 B/row -- by ten coalesced nontemporal 8-byte loads per lane
//     and row into a wave-private LDS strip (the row-lds kernel's layout: row j of the tile at strip position 5 (j - j0), [N,W,C,E,S];
//     column 0 holds [N,C,E,S] at positions 1..4), addresses clamped at the array's ends, where the slots feed no row;
//   * z on the four grid rows 2I-1 .. 2I+2 and r on the two rows, a 16-byte pair per lane and row where the pair is 16-byte aligned
//     (an odd n leaves the odd grid rows 8-byte aligned only: two 8-byte loads there) -- every load is issued before the first use;
//   * the W neighbour of ja and the E neighbour of jb from the adjacent lanes (a cross-lane move); only lane 0 and lane 63 load an outer
//     column;
//   * the row sums through stencil5_row's chains, t = fma(-1.0, sum, r), r_c = ((t00 + t01) + t10) + t11 over the members that exist;
//   * one plain 8-byte store per lane: the next level reads it at once.
// Unique bytes per fine row: 40 + 8 + 8 + 2. A pair that holds grid row 0 or n-1, and a lone last grid row, go one thread per
// aggregate without the strip (residual_off_tile): grid rows 0 and n-1 walk the CSR in loop order (sum = 0 ; sum = fma(v[k],
// z[col[k]], sum), ascending k), their interior partner takes its chain -- the bits stencil5-csr's SpMV gives for each row.
// Tiles are dealt to the XCDs in runs (xcd_run_tile); the launcher pads the grid.

// store_strip5, strip_row, load_pair and residual_off_tile: multigrid_device.hpp
__global__ __launch_bounds__(kWave) void residual_restrict_kernel(SlabCsr m, const double* __restrict__ z, const double* __restrict__ r,
                                                                  double* __restrict__ rc, int nc, int col_tiles, int total_tiles, int run) {
    __shared__ double strip[2][5 * kStripCols];
    const int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    const int n = m.grid_size;
    const int I = tile / col_tiles;
    const int j0 = (tile - I * col_tiles) * kStripCols;
    const int lane = (int)threadIdx.x;
    const int ja = j0 + 2 * lane, jb = ja + 1;
    const int i0 = 2 * I, i1 = i0 + 1;
    const bool has_a = ja < n, has_b = jb < n;
    if (i0 >= 1 && i1 <= n - 2) {
        // every load of the tile, then the first use
        double c[2][10];
        const long long hi = m.nnz_local - 1;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const long long e = stencil_gridrow_base(i0 + a, n) + 5LL * j0 - 1 + lane;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                long long idx = e + 64 * k;
                idx = idx < 0 ? 0 : (idx > hi ? hi : idx);
                c[a][k] = __builtin_nontemporal_load(m.values + idx);
            }
        }
        d2 zv[4], rv[2];
        double west[2] = {0.0, 0.0}, east[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) zv[q] = d2{0.0, 0.0};
        rv[0] = rv[1] = d2{0.0, 0.0};
        if (has_a) {
#pragma unroll
            for (int q = 0; q < 4; ++q) zv[q] = load_pair<false>(z, (long long)(i0 - 1 + q) * n + ja, has_b);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                rv[a] = load_pair<true>(r, (long long)(i0 + a) * n + ja, has_b);
                if (lane == 0 && ja > 0) west[a] = z[(long long)(i0 + a) * n + ja - 1];
                if (lane == 63 && jb + 1 < n) east[a] = z[(long long)(i0 + a) * n + jb + 1];
            }
        }
        store_strip5(strip, lane, c);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const d2 zc = zv[1 + a], zn = zv[a], zs = zv[2 + a];
            const double from_west = __shfl_up(zc.y, 1), from_east = __shfl_down(zc.x, 1);
            const double xw_a = lane > 0 ? from_west : west[a];
            const double xe_b = lane < 63 ? from_east : east[a];
            if (has_a) {
                const double* __restrict__ v = strip[a] + 5 * (2 * lane);
                const double ta = fma(-1.0, strip_row(v, ja, n, xw_a, zc.x, zc.y, zn.x, zs.x), rv[a].x);
                acc = a == 0 ? ta : acc + ta;
                if (has_b) {
                    const double tb = fma(-1.0, strip_row(v + 5, jb, n, zc.x, zc.y, xe_b, zn.y, zs.y), rv[a].y);
                    acc = acc + tb;
                }
            }
        }
        if (has_a) rc[(long long)I * nc + (ja >> 1)] = acc;
    } else if (has_a) {
        // a pair with grid row 0 or n-1 in it, a lone last grid row
        double acc = residual_off_tile(m, z, r, i0, ja);
        if (has_b) acc = acc + residual_off_tile(m, z, r, i0, jb);
        if (i1 < n) {
            acc = acc + residual_off_tile(m, z, r, i1, ja);
            if (has_b) acc = acc + residual_off_tile(m, z, r, i1, jb);
        }
        rc[(long long)I * nc + (ja >> 1)] = acc;
    }
}

// ---- prolongation + correction: z = fma(2.0, e_c[agg(i)], z), z in place; one-wave workgroups, a 16-byte pair per lane ----
// coarse_at (multigrid_device.hpp): e_c at the aggregate of a flat fine row
__global__ __launch_bounds__(kWave) void prolong_correct_kernel(size_t rows, int n, int nc, const double* __restrict__ ec, double* __restrict__ z) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < (rows >> 1)) {
        d2 zv = reinterpret_cast<const d2*>(z)[i];
        zv.x = fma(2.0, coarse_at(ec, 2 * i, n, nc), zv.x);
        zv.y = fma(2.0, coarse_at(ec, 2 * i + 1, n, nc), zv.y);
        reinterpret_cast<d2*>(z)[i] = zv;  // plain: the post-smoother's SpMV reads it
    }
    if ((rows & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[rows - 1] = fma(2.0, coarse_at(ec, rows - 1, n, nc), z[rows - 1]);
}

}  // namespace

// ---- the launches (multigrid.hpp) ----
namespace spmv_amd {

void launch_coarsen(const SlabCsr& fine, int nc, int* row_ptr, int* col_idx, double* values) {
    const int rows = nc * nc;
    hipLaunchKernelGGL(coarsen_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, kStream, fine, fine.grid_size, nc, row_ptr, col_idx, values);
}

void launch_residual_restrict(const SlabCsr& m, const double* z, const double* r, double* rc) {
    const RestrictTiles t = restrict_tiles5(m.grid_size);
    hipLaunchKernelGGL(residual_restrict_kernel, dim3(t.grid()), dim3(kWave), 0, kStream, m, z, r, rc, t.nc, t.col_tiles, t.tiles, t.run);
}

void launch_prolong_correct(int n, const double* ec, double* z) {
    const size_t rows = (size_t)n * n;
    hipLaunchKernelGGL(prolong_correct_kernel, dim3(stream_grid(rows)), dim3(kWave), 0, kStream, rows, n, coarse_grid_of(n), ec, z);
}

SlabCsr mg_stencil_view(int n, const int* row_ptr, const int* col_idx, const double* values) {
    SlabCsr v;
    v.row_ptr = row_ptr, v.col_idx = col_idx, v.values = values;
    v.n_local = v.n_global = n * n;
    v.nnz_local = stencil_nnz(n);
    v.max_row_nnz = n >= 3 ? 5 : (n == 2 ? 3 : 1);
    v.grid_size = n;
    return v;
}

void mg_destroy(MgHierarchy* h) {
    if (h == nullptr) return;
    h->release();
    delete h;
}

double* mg_result_vector(MgHierarchy* h) { return h->levels[0].z; }
MgMulti* mg_multi_of(const MgHierarchy* h) { return h != nullptr ? h->multi : nullptr; }
bool mg_verify_stencil5(SlabCsr& v) { return verified(v); }
bool mg_verify_stencil7(SlabCsr& v, int n) { return verified(v, 3, n); }

namespace {

// The single-vector cycle's operations (mg_schedule.hpp): section 14's application per level, a ChebRun whose z and aux change places
// on fused levels. A launch that carries a product counts as SpMV time, every other as BLAS1.
struct CycleOps {
    MgHierarchy* h;
    const double* r;  // level 0's
    StageTimers* T;
    ChebRun run[kMaxLevels];

    void term0(int l) {
        MgLevel& L = h->levels[(size_t)l];
        ChebRun& c = run[l];  // only a last step of level 0 writes partials
        c.a = L.spmv(), c.n = (size_t)L.rows, c.r = l == 0 ? r : L.r, c.dinv = L.dinv, c.d = L.d, c.z = L.z, c.aux = L.aux, c.partials = h->partials, c.T = T;
        stage_run(T, &StageTimers::t_blas, [&] { launch_cheb_term0_apply(c.n, c.r, L.dinv, L.coef[0], L.d, c.z); });
    }
    void step(int l, double g, double hh, bool last) { (void)cheb_step(run[l], g, hh, last); }  // no run_device here
    void restrict_residual(int l) {
        const MgLevel& L = h->levels[(size_t)l];
        double* const rc = h->levels[(size_t)l + 1].r;
        stage_run(T, &StageTimers::t_spmv, [&] {
            if (L.dim == 0) launch_amg_residual_restrict(L.view, L.coarse_rows, L.agg_ptr, L.members, run[l].z, run[l].r, rc);
            else if (L.dim == 3) launch_residual_restrict3d(L.view, L.n, run[l].z, run[l].r, rc);
            else launch_residual_restrict(L.view, run[l].z, run[l].r, rc);
        });
    }
    void prolong(int l) {
        const MgLevel& L = h->levels[(size_t)l];
        stage_run(T, &StageTimers::t_blas, [&] {
            if (L.dim == 0) launch_amg_prolong_correct((size_t)L.rows, L.agg, run[l + 1].z, run[l].z);
            else if (L.dim == 3) launch_prolong_correct3d(L.n, run[l + 1].z, run[l].z);
            else launch_prolong_correct(L.n, run[l + 1].z, run[l].z);
        });
    }
};

}  // namespace

Applied mg_cycle(MgHierarchy* h, const double* r, StageTimers* T) {
    CycleOps ops{h, r, T, {}};
    mg_vcycle(ops, h->levels.data(), h->count());
    const ChebRun& top = ops.run[0];  // level 0's z and the r.z partials of its last step
    return Applied{top.z, top.rz_partials, top.rz_count};
}

}  // namespace spmv_amd

namespace {

// Builds level l (> 0) of the hierarchy from level l - 1, or level 0 from the operator's view; false = refused (said on stderr).
bool finish_level(MgHierarchy* h, int l, const LaunchShape& shape, int* bad_row) {
    MgLevel& L = h->levels[(size_t)l];
    const bool coarsest = l + 1 == (int)h->levels.size();
    if (l > 0) {
        const MgLevel& F = h->levels[(size_t)l - 1];
        L.A.allocate((size_t)L.rows, (size_t)L.nnz());
        if (L.dim == 3) {
            launch_coarsen3d(F.view, F.n, L.A.row_ptr, L.A.col_idx, L.A.values);
            L.A.view = stencil7_view(L.n, L.A.row_ptr, L.A.col_idx, L.A.values);
        } else {
            launch_coarsen(F.view, L.n, L.A.row_ptr, L.A.col_idx, L.A.values);
            L.A.view = mg_stencil_view(L.n, L.A.row_ptr, L.A.col_idx, L.A.values);
        }
        HIP_CHECK(hipGetLastError());
        L.view = L.A.view;
        if (!verified(L.view, L.dim, L.n)) {
            fprintf(stderr, "[PCG] multigrid: the coarse operator of level %d is not a complete %d-point stencil: refused\n", l, L.dim == 3 ? 7 : 5);
            return false;
        }
        L.A.view = L.view;
        char who[40];
        snprintf(who, sizeof who, "multigrid: level %d", l);
        L.dinv = inverse_diagonal_of_csr(L.view, L.rows, who, bad_row);
        if (L.dinv == nullptr) return false;
    }
    L.lambda_max = gershgorin_of_csr(L.view, L.rows, L.dinv);
    const double lmin = coarsest ? L.lambda_max / 30.0 : L.lambda_max / 4.0;
    if (!isfinite(L.lambda_max) || !(lmin > 0.0) || !(lmin < L.lambda_max)) {
        fprintf(stderr, "[PCG] multigrid: level %d: the interval [%g, %g] is not 0 < lambda_min < lambda_max, both finite: refused\n", l, lmin,
                L.lambda_max);
        return false;
    }
    L.degree = coarsest ? kMgCoarsestDegree : h->smoother_degree;
    chebyshev_coefficients(L.degree, lmin, L.lambda_max, L.coef);
    if (L.dim == 3) L.plan7 = plan_stencil7(L.view, L.n, true, Stencil7Variant::Auto, shape.knobs);  // row-lds from the knob's grid, row-direct below
    else L.plan = plan_stencil5(L.view, 0, L.rows, Stencil5Variant::Auto, shape);
    if (l > 0) L.r = device_try_alloc<double>((size_t)L.rows);
    L.d = device_try_alloc<double>((size_t)L.rows);
    L.z = device_try_alloc<double>((size_t)L.rows);
    L.aux = device_try_alloc<double>((size_t)L.rows);
    if ((l > 0 && L.r == nullptr) || L.d == nullptr || L.z == nullptr || L.aux == nullptr) return fail("the level vectors could not be allocated: refused");
    return true;
}

// The one creator: dim 2 for stencil5-csr (spmv_amd_precond_create_multigrid), dim 3 for stencil7-csr (..._multigrid3d). max_rhs > 0
// (..._multigrid_multi, ..._multigrid3d_multi): the hierarchy also gets block vectors of that many columns and an SpMM plan on every level.
SpmvAmdPrecond* create_multigrid(SpmvOperator* op, int dim, int smoother_degree, int max_levels, int* bad_row, int max_rhs = 0) {
    // argument checks: all before the first HIP call
    if (bad_row != nullptr) *bad_row = -1;
    if (op == nullptr) return fail("null operator"), nullptr;
    if (smoother_degree < 0 || smoother_degree > kMaxSmoother) {
        fprintf(stderr, "[PCG] multigrid: smoother degree %d is outside 0..%d: refused\n", smoother_degree, kMaxSmoother);
        return nullptr;
    }
    if (max_levels < 0 || max_levels > kMaxLevels) {
        fprintf(stderr, "[PCG] multigrid: max_levels %d is neither 0 (automatic) nor 1..%d: refused\n", max_levels, kMaxLevels);
        return nullptr;
    }
    DiagonalSource d;
    if (!creation_source(op, "multigrid: ", dim == 3 ? "stencil7-csr: refused" : "stencil5-csr: refused", /*stencil_dim=*/dim, &d)) return nullptr;
    int n0 = 0;
    if (dim == 3) {
        const Stencil7Source s7 = stencil7_source_of(op);  // the 3-D geometry lives in the operator, not in the view
        n0 = s7.grid;
        if (!s7.verified || s7.csr_loop || n0 < 2 || d.rows != d.cols || (long long)n0 * n0 * n0 != d.rows) {
            fprintf(stderr, "[PCG] multigrid: operator '%s' does not run a verified complete 7-point stencil (its plan is %s): refused\n", op->name,
                    s7.plan_name);
            return nullptr;
        }
    } else {
        n0 = d.csr.grid_size;
        if (!d.csr.verified_stencil || n0 < 1 || d.rows != d.cols || (long long)n0 * n0 != d.rows) {
            fprintf(stderr, "[PCG] multigrid: the matrix of operator '%s' is not a verified complete 5-point stencil: refused\n", op->name);
            return nullptr;
        }
    }

    MgHierarchy* h = new MgHierarchy();
    h->dim = dim;
    h->smoother_degree = smoother_degree;
    size_t need = 0;
    for (int n = n0;; n = coarse_grid_of(n)) {
        MgLevel L;
        L.dim = dim, L.n = n, L.rows = dim == 3 ? n * n * n : n * n;
        const bool top = h->levels.empty();
        h->levels.push_back(L);
        need += (size_t)L.rows * sizeof(double) * (top ? 3 : 5);
        if (!top) need += (size_t)L.nnz() * (sizeof(double) + sizeof(int)) + ((size_t)L.rows + 1) * sizeof(int) + 3 * 4096;
        if (n <= kCoarsestGrid || (max_levels > 0 && (int)h->levels.size() == max_levels)) break;
    }
    SpmvAmdPrecond* pm = nullptr;
    char what[64];
    snprintf(what, sizeof what, "%d levels on %d rows (multigrid)", (int)h->levels.size(), d.rows);
    const LaunchShape shape = current_launch_shape();
    if (max_rhs > 0) need += mg_multi_bytes(h, max_rhs);
    bool ok = device_has_room(need + (size_t)d.rows * sizeof(double) + ((size_t)64 << 20), "PCG", what);
    if (ok) {
        MgLevel& top = h->levels[0];
        top.view = d.csr;
        top.own_dinv = false;
        top.dinv = inverse_diagonal_of_csr(top.view, top.rows, "multigrid: level 0", bad_row);
        if (top.dinv == nullptr) {
            ok = false;
        } else {
            pm = new SpmvAmdPrecond();
            pm->kind = kMultigrid;
            pm->n = d.rows;
            pm->dinv = top.dinv;
            pm->degree = smoother_degree;
            pm->owner = d.owner;
            pm->generation = d.generation;
        }
    }
    for (int l = 0; ok && l < (int)h->levels.size(); ++l) ok = finish_level(h, l, shape, bad_row);
    if (ok) {
        const MgLevel& top = h->levels[0];
        const size_t slots = top.fused() ? (size_t)top.plan.partials : (size_t)stream_grid((size_t)top.rows);
        h->partials = device_try_alloc<double>(slots);
        if (h->partials == nullptr) ok = fail("the partials could not be allocated: refused");
    }
    if (ok && max_rhs > 0) {
        h->multi = mg_multi_create(h, max_rhs);
        ok = h->multi != nullptr;
    }
    HIP_CHECK(hipStreamSynchronize(kStream));
    if (!ok) {
        mg_destroy(h);
        if (pm != nullptr) {
            device_release(pm->dinv);
            delete pm;
        }
        return nullptr;
    }
    pm->mg = h;
    pm->lambda_max = h->levels[0].lambda_max;
    pm->lambda_min = pm->lambda_max / (h->levels.size() == 1 ? 30.0 : 4.0);
    return pm;
}

}  // namespace

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_multigrid(SpmvOperator* op, int smoother_degree, int max_levels, int* bad_row) {
    return create_multigrid(op, 2, smoother_degree, max_levels, bad_row);
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_multigrid3d(SpmvOperator* op, int smoother_degree, int max_levels, int* bad_row) {
    return create_multigrid(op, 3, smoother_degree, max_levels, bad_row);
}

// what the two block creators check of max_rhs: before any HIP call, like the creator's other argument checks
static bool max_rhs_in_range(int max_rhs, int* bad_row) {
    if (max_rhs >= 1 && max_rhs <= kMaxRhs) return true;
    if (bad_row != nullptr) *bad_row = -1;
    fprintf(stderr, "[PCG] multigrid: max_rhs %d is outside 1..%d: refused\n", max_rhs, kMaxRhs);
    return false;
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_multigrid_multi(SpmvOperator* op, int smoother_degree, int max_levels, int max_rhs,
                                                                   int* bad_row) {
    if (!max_rhs_in_range(max_rhs, bad_row)) return nullptr;
    return create_multigrid(op, 2, smoother_degree, max_levels, bad_row, max_rhs);
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_multigrid3d_multi(SpmvOperator* op, int smoother_degree, int max_levels, int max_rhs,
                                                                     int* bad_row) {
    if (!max_rhs_in_range(max_rhs, bad_row)) return nullptr;
    return create_multigrid(op, 3, smoother_degree, max_levels, bad_row, max_rhs);
}

extern "C" int spmv_amd_precond_multigrid_max_rhs(const SpmvAmdPrecond* m) {
    return m != nullptr && m->kind == kMultigrid ? mg_multi_capacity(mg_multi_of(m->mg)) : 0;
}

extern "C" int spmv_amd_precond_multigrid_dimension(const SpmvAmdPrecond* m) {
    return m != nullptr && m->kind == kMultigrid && m->mg != nullptr ? m->mg->dim : 0;
}

extern "C" int spmv_amd_precond_multigrid_info(const SpmvAmdPrecond* m, int* levels, int* smoother_degree, int* grids, double* lambda_max, int cap) {
    if (m == nullptr || m->kind != kMultigrid || m->mg == nullptr) return 0;
    const int count = (int)m->mg->levels.size();
    if (levels != nullptr) *levels = count;
    if (smoother_degree != nullptr) *smoother_degree = m->mg->smoother_degree;
    for (int l = 0; l < count && l < cap; ++l) {
        if (grids != nullptr) grids[l] = m->mg->levels[(size_t)l].n;
        if (lambda_max != nullptr) lambda_max[l] = m->mg->levels[(size_t)l].lambda_max;
    }
    return count;
}

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_precond_multigrid_level_csr(const SpmvAmdPrecond* m, int level, int* row_ptr, int* col_idx, double* values, double* dinv) {
    if (m == nullptr || m->kind != kMultigrid || m->mg == nullptr) return fail("level_csr: not a multigrid preconditioner"), 1;
    if (level < 0 || level >= (int)m->mg->levels.size()) return fail("level_csr: no such level"), 1;
    const MgLevel& L = m->mg->levels[(size_t)level];
    HIP_CHECK(hipStreamSynchronize(kStream));
    if (row_ptr != nullptr) download(row_ptr, L.view.row_ptr, (size_t)L.rows + 1);
    if (col_idx != nullptr) download(col_idx, L.view.col_idx, (size_t)L.view.nnz_local);
    if (values != nullptr) download(values, L.view.values, (size_t)L.view.nnz_local);
    if (dinv != nullptr) download(dinv, L.dinv, (size_t)L.rows);
    return 0;
}

extern "C" int spmv_amd_mg_stage(const char* stage, SpmvAmdMgStageArgs* a) {
    // argument checks: all before the first HIP call
    enum Stage { kCoarsen, kRestrict, kProlong };
    static const struct {
        const char* name;
        Stage st;
        int dim;
    } kStages[] = {{"coarsen", kCoarsen, 2},   {"residual_restrict", kRestrict, 2},   {"prolong", kProlong, 2},
                   {"coarsen3d", kCoarsen, 3}, {"residual_restrict3d", kRestrict, 3}, {"prolong3d", kProlong, 3}};
    if (stage == nullptr) return fail("stage: none named (coarsen, residual_restrict, prolong, and each with the suffix 3d)"), 1;
    Stage st = kCoarsen;
    int dim = 0;
    for (const auto& known : kStages)
        if (!strcmp(stage, known.name)) st = known.st, dim = known.dim;
    if (dim == 0) return fail("stage: unknown (coarsen, residual_restrict, prolong, and each with the suffix 3d)"), 1;
    if (a == nullptr) return fail("stage: null arguments"), 1;
    if (dim == 2 && (a->n < 2 || a->n > 46340)) return fail("stage: the fine grid is outside 2..46340"), 1;
    if (dim == 3 && (a->n < 2 || a->n > kStencil7MaxGrid)) return fail("stage: the fine grid of a 3-D stage is outside 2..674"), 1;
    const auto aligned = [](const void* p, uintptr_t to) { return p != nullptr && ((uintptr_t)p & (to - 1)) == 0; };
    if (st != kProlong && (!aligned(a->row_ptr, 4) || !aligned(a->col_idx, 4) || !aligned(a->values, 8)))
        return fail("stage: a null or misaligned CSR array"), 1;
    if (st == kCoarsen && (!aligned(a->out_row_ptr, 4) || !aligned(a->out_col_idx, 4) || !aligned(a->out_values, 8)))
        return fail("stage: a null or misaligned coarse CSR array"), 1;
    if (st == kRestrict && (!aligned(a->z, 16) || !aligned(a->r, 16) || !aligned(a->coarse, 8)))
        return fail("stage: z and r must be 16-byte aligned, the coarse vector 8-byte aligned"), 1;
    if (st == kProlong && (!aligned(a->z, 16) || !aligned(a->coarse, 8)))
        return fail("stage: z must be 16-byte aligned, the coarse vector 8-byte aligned"), 1;

    if (st == kProlong) {
        if (dim == 3) launch_prolong_correct3d(a->n, a->coarse, a->z);
        else launch_prolong_correct(a->n, a->coarse, a->z);
    } else if (dim == 3) {
        SlabCsr fine = stencil7_view(a->n, a->row_ptr, a->col_idx, a->values);
        if (!verified(fine, 3, a->n)) return fail("stage: the CSR is not a complete 7-point stencil of that grid: refused"), 1;
        if (st == kCoarsen) launch_coarsen3d(fine, a->n, a->out_row_ptr, a->out_col_idx, a->out_values);
        else launch_residual_restrict3d(fine, a->n, a->z, a->r, a->coarse);
    } else {
        SlabCsr fine = mg_stencil_view(a->n, a->row_ptr, a->col_idx, a->values);
        if (!verified(fine)) return fail("stage: the CSR is not a complete 5-point stencil of that grid: refused"), 1;
        if (st == kCoarsen) launch_coarsen(fine, coarse_grid_of(a->n), a->out_row_ptr, a->out_col_idx, a->out_values);
        else launch_residual_restrict(fine, a->z, a->r, a->coarse);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}
#endif  // SPMV_AMD_LAB
