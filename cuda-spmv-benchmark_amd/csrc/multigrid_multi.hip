// multigrid_multi.hip -- kind "multigrid" of the batched preconditioned solver (pcg_multi.hip): the V(nu, nu) cycle of multigrid.hip on
// block vectors of up to 8 interleaved columns (multi_rhs.hpp), for the 2-D hierarchy of stencil5-csr (DESIGN.md section 19;
// include/spmv_amd/api.h states the algebra) and, with the restriction and prolongation of multigrid3d_multi.hip in the place of the two
// here, for the 3-D hierarchy of stencil7-csr (spmv_amd_precond_create_multigrid3d_multi). The hierarchy, its coarse operators, dinv, bounds and coefficients are multigrid.hip's;
// spmv_amd_precond_create_multigrid_multi adds what is here: on every level above 0 the block vectors R, D, Z and W of max_rhs columns,
// and on every level an SpmmPlan on the level's own view and Stencil5Plan variant (a 3-D level: "spmm/csr"). Level 0 works on its caller's vectors -- the solve's
// R, D, Z and AP buffer, or the block application's. An AMG hierarchy (spmv_amd_precond_create_amg_multi) runs the
// same cycle: its levels have dim == 0, their plan is "spmm/csr" and their two transfers are amg_multi.hip's.
//
// The cycle is mg_schedule.hpp's mg_vcycle with the operations of MultiOps below; the levels are read straight from multigrid.hpp's
// MgHierarchy. A cycle's launch count does not depend on k: the columns share every launch, and the three launches that are
// multigrid's own read what the columns share once --
//   residual_restrict_multi_kernel<K>  r_c[I, J][j] = ((t00 + t01) + t10) + t11 per column, t = fma(-1.0, (A z)_i, r_i): the two rows'
//                                      coefficients go through the wave-private LDS strip once for all K columns
//   prolong_correct_multi_kernel<K>    z[i][j] = fma(2.0, e_c[agg(i)][j], z[i][j]), flat over rows x columns
//   mg_multi_term0_kernel<K>           d = c0 * (dinv * r) ; z = d on the levels above 0 (level 0's term 0 is written by the solve's r update)
// A smoothing step is launch_spmm on the level's plan into W and pcg_multi.hip's step kernel (launch_pcg_multi_cheb_step).
// Per column every result has the bits of multigrid.hip's single-vector cycle: the SpMM gives the operator's own product bits, the
// kernels here evaluate multigrid.hip's expressions per column. Every kernel reads the column records first and returns when no column
// is running (null records: all are); a stopped column beside running ones is computed like them -- D, Z and the level vectors are
// scratch for it.
// Indices: a row index times K is formed in 64 bits everywhere (4e8 rows x 8 columns pass int).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "mg_schedule.hpp"
#include "multi_rhs.hpp"
#include "multi_solve.hpp"
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

constexpr const char* kTag = "PCG-MULTI";
constexpr int kWave = 64;
constexpr int kChunk = 4;  // columns one pass of the restriction holds in registers: 12 * 4 doubles of z and r per lane

// store_strip5, strip_row, residual_off_tile<K>, any_running, load_run, store_run and the flat walk: multigrid_device.hpp

// ---- residual + restriction in one launch, K columns ----
// The tile, the strip, the fast-path test, the off-tile path and the XCD deal are residual_restrict_kernel's (multigrid.hip). A lane's
// fine pair (ja, ja + 1) of one grid row is 2 K contiguous doubles. The columns are walked in chunks of at most 4: one chunk's z on the
// four grid rows and r on the two -- 12 * 4 doubles per lane, every load issued before the first use -- stay in registers while the strip
// stays where it is; at K = 8 all 96 doubles at once would leave no room beside the coefficients.
// Unique bytes per fine row: 40 (coefficients, once) + K (8 + 8 + 2).

template <int C>
struct RestrictRegs {
    double za[4][C], zb[4][C];  // z at columns ja / ja + 1 on the grid rows i0 - 1 .. i0 + 2
    double ra[2][C], rb[2][C];
    double west[2][C], east[2][C];  // lane 0's W neighbour of ja, lane 63's E neighbour of ja + 1
};

template <int K, int C0, int C>
__device__ __forceinline__ void restrict_load(RestrictRegs<C>& t, const double* __restrict__ z, const double* __restrict__ r, int n, int i0,
                                              int ja, int lane, bool has_a, bool has_b) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
#pragma unroll
        for (int g = 0; g < 4; ++g) t.za[g][q] = t.zb[g][q] = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a) t.ra[a][q] = t.rb[a][q] = t.west[a][q] = t.east[a][q] = 0.0;
    }
    if (!has_a) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long long at = ((long long)(i0 - 1 + g) * n + ja) * K + C0;
        load_run<C, false>(z + at, t.za[g]);
        if (has_b) load_run<C, false>(z + at + K, t.zb[g]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const long long at = ((long long)(i0 + a) * n + ja) * K + C0;
        load_run<C, true>(r + at, t.ra[a]);
        if (has_b) load_run<C, true>(r + at + K, t.rb[a]);
        if (lane == 0 && ja > 0) load_run<C, false>(z + at - K, t.west[a]);
        if (lane == 63 && ja + 2 < n) load_run<C, false>(z + at + 2 * K, t.east[a]);
    }
}

template <int K, int C0, int C>
__device__ __forceinline__ void restrict_sum(const RestrictRegs<C>& t, const double (*strip)[5 * kStripCols], double* __restrict__ rc, int n,
                                             int nc, int I, int ja, int lane, bool has_a, bool has_b) {
    double acc[C];
#pragma unroll
    for (int q = 0; q < C; ++q) acc[q] = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double* __restrict__ v = strip[a] + 5 * (2 * lane);
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const double zx = t.za[1 + a][q], zy = t.zb[1 + a][q];
            const double from_west = __shfl_up(zy, 1), from_east = __shfl_down(zx, 1);
            const double xw_a = lane > 0 ? from_west : t.west[a][q];
            const double xe_b = lane < 63 ? from_east : t.east[a][q];
            if (has_a) {
                const double ta = fma(-1.0, strip_row(v, ja, n, xw_a, zx, zy, t.za[a][q], t.za[2 + a][q]), t.ra[a][q]);
                acc[q] = a == 0 ? ta : acc[q] + ta;
                if (has_b) {
                    const double tb = fma(-1.0, strip_row(v + 5, ja + 1, n, zx, zy, xe_b, t.zb[a][q], t.zb[2 + a][q]), t.rb[a][q]);
                    acc[q] = acc[q] + tb;
                }
            }
        }
    }
    if (has_a) store_run<C>(rc + ((long long)I * nc + (ja >> 1)) * K + C0, acc);
}

// the chunks behind the first: columns C0 .. K - 1, the strip already in LDS
template <int K, int C0>
__device__ __forceinline__ void restrict_rest(const double (*strip)[5 * kStripCols], const double* __restrict__ z, const double* __restrict__ r,
                                              double* __restrict__ rc, int n, int nc, int I, int i0, int ja, int lane, bool has_a, bool has_b) {
    if constexpr (C0 < K) {
        constexpr int C = K - C0 < kChunk ? K - C0 : kChunk;
        RestrictRegs<C> next;
        restrict_load<K, C0, C>(next, z, r, n, i0, ja, lane, has_a, has_b);
        restrict_sum<K, C0, C>(next, strip, rc, n, nc, I, ja, lane, has_a, has_b);
        restrict_rest<K, C0 + C>(strip, z, r, rc, n, nc, I, i0, ja, lane, has_a, has_b);
    }
}

template <int K>
__global__ __launch_bounds__(kWave) void residual_restrict_multi_kernel(SlabCsr m, const PcgMultiColumn* __restrict__ cols,
                                                                        const double* __restrict__ z, const double* __restrict__ r,
                                                                        double* __restrict__ rc, int nc, int col_tiles, int total_tiles, int run) {
    __shared__ double strip[2][5 * kStripCols];
    if (!any_running<K>(cols)) return;  // uniform over the launch
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
        // the coefficients of the two rows and the first chunk's z and r: every load, then the first use
        constexpr int CA = K < kChunk ? K : kChunk;
        double c[2][10];
        const long long hi = m.nnz_local - 1;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const long long e = stencil_gridrow_base(i0 + a, n) + 5LL * j0 - 1 + lane;
#pragma unroll
            for (int s = 0; s < 10; ++s) {
                long long idx = e + 64 * s;
                idx = idx < 0 ? 0 : (idx > hi ? hi : idx);
                c[a][s] = __builtin_nontemporal_load(m.values + idx);
            }
        }
        RestrictRegs<CA> first;
        restrict_load<K, 0, CA>(first, z, r, n, i0, ja, lane, has_a, has_b);
        store_strip5(strip, lane, c);
        restrict_sum<K, 0, CA>(first, strip, rc, n, nc, I, ja, lane, has_a, has_b);
        restrict_rest<K, CA>(strip, z, r, rc, n, nc, I, i0, ja, lane, has_a, has_b);
    } else if (has_a) {
        // a pair with grid row 0 or n-1 in it, a lone last grid row
#pragma unroll
        for (int q = 0; q < K; ++q) {
            double acc = residual_off_tile<K, long long>(m, z, r, i0, ja, q);
            if (has_b) acc = acc + residual_off_tile<K, long long>(m, z, r, i0, jb, q);
            if (i1 < n) {
                acc = acc + residual_off_tile<K, long long>(m, z, r, i1, ja, q);
                if (has_b) acc = acc + residual_off_tile<K, long long>(m, z, r, i1, jb, q);
            }
            rc[((long long)I * nc + (ja >> 1)) * K + q] = acc;
        }
    }
}

// ---- the flat kernels (FlatWalk, multigrid_device.hpp) ----
// z[i][j] = fma(2.0, e_c[agg(i)][j], z[i][j]), z in place
template <int K>
__global__ __launch_bounds__(kFlat) void prolong_correct_multi_kernel(long long rows, int n, int nc, const PcgMultiColumn* __restrict__ cols,
                                                                      const double* __restrict__ ec, double* __restrict__ z) {
    constexpr int V = FlatWalk<K>::V, U = FlatWalk<K>::P;
    if (!any_running<K>(cols)) return;
    const long long row0 = (long long)blockIdx.x * kFlat;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kFlat * i;
        const int t = f / U, col0 = (f - t * U) * V;
        const long long row = row0 + t;
        if (row >= rows) continue;
        const int gi = (int)(row / n), gj = (int)(row - (long long)gi * n);
        const long long coarse = (long long)(gi >> 1) * nc + (gj >> 1);
        double zv[V], ev[V];
        load_unit<V>(z + row * K + col0, zv);
        load_unit<V>(ec + coarse * K + col0, ev);
#pragma unroll
        for (int q = 0; q < V; ++q) zv[q] = fma(2.0, ev[q], zv[q]);
        store_unit<V>(z + row * K + col0, zv);
    }
}

// term 0 of a level above 0: u = dinv r ; d = c0 u ; z = d (D may be null: the block application's Jacobi form, c0 = 1.0)
template <int K>
__global__ __launch_bounds__(kFlat) void mg_multi_term0_kernel(long long rows, const PcgMultiColumn* __restrict__ cols, const double* __restrict__ R,
                                                               const double* __restrict__ dinv, double c0, double* __restrict__ D,
                                                               double* __restrict__ Z) {
    constexpr int V = FlatWalk<K>::V, U = FlatWalk<K>::P;
    if (!any_running<K>(cols)) return;
    const long long row0 = (long long)blockIdx.x * kFlat;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kFlat * i;
        const int t = f / U, col0 = (f - t * U) * V;
        const long long row = row0 + t;
        if (row >= rows) continue;
        double v[V];
        load_unit<V>(R + row * K + col0, v);
        const double dv = dinv[row];
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = c0 * (dv * v[q]);
        if (D != nullptr) store_unit<V>(D + row * K + col0, v);
        store_unit<V>(Z + row * K + col0, v);
    }
}

unsigned flat_grid(long long rows) { return (unsigned)((rows + kFlat - 1) / kFlat); }

}  // namespace

// ---- the launches (multigrid.hpp) ----
void spmv_amd::launch_residual_restrict_multi(int k, const SlabCsr& m, const PcgMultiColumn* cols, const double* z, const double* r, double* rc) {
    const RestrictTiles t = restrict_tiles5(m.grid_size);
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((residual_restrict_multi_kernel<decltype(K)::value>), dim3(t.grid()), dim3(kWave), 0, kBatchStream, m, cols, z, r, rc, t.nc,
                           t.col_tiles, t.tiles, t.run);
    });
}

void spmv_amd::launch_prolong_correct_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z) {
    const long long rows = (long long)n * n;
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((prolong_correct_multi_kernel<decltype(K)::value>), dim3(flat_grid(rows)), dim3(kFlat), 0, kBatchStream, rows, n,
                           coarse_grid_of(n), cols, ec, z);
    });
}

// multi_rhs.hpp: the batched GCR solver (gcr_multi.hip) launches term 0 of its applications with it too
void spmv_amd::launch_mg_multi_term0(int k, long long rows, const PcgMultiColumn* cols, const double* R, const double* dinv, double c0, double* D,
                                     double* Z) {
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((mg_multi_term0_kernel<decltype(K)::value>), dim3(flat_grid(rows)), dim3(kFlat), 0, kBatchStream, rows, cols, R, dinv, c0,
                           D, Z);
    });
}

namespace {

bool fail(const char* what) { return batched_fail(kTag, what); }

}  // namespace

namespace spmv_amd {

struct MgMulti {
    struct Level {
        double *R = nullptr, *D = nullptr, *Z = nullptr, *W = nullptr;  // levels above 0: rows x max_rhs each
        SpmmPlan plan;
    };
    int max_rhs = 0;
    std::vector<Level> levels;
};

int mg_multi_capacity(const MgMulti* mm) { return mm != nullptr ? mm->max_rhs : 0; }

size_t mg_multi_bytes(const MgHierarchy* h, int max_rhs) {
    size_t bytes = 0;
    for (int l = 1; l < h->count(); ++l) bytes += 4 * (size_t)h->levels[(size_t)l].rows * (size_t)max_rhs * sizeof(double) + 4 * 4096;
    return bytes;
}

void mg_multi_destroy(MgMulti* mm) {
    if (mm == nullptr) return;
    for (MgMulti::Level& L : mm->levels) {
        device_release(L.R);
        device_release(L.D);
        device_release(L.Z);
        device_release(L.W);
    }
    delete mm;
}

// A 3-D level's block product: "spmm/stencil7-row-lds" (stencil7_spmm.hip) from this grid upward, below it the generic CSR gather
// "spmm/csr" -- the kind of the operator's own multi-RHS plan on stencil7-csr. Both give the same bits. The LAB build can force either
// kind on every level of the hierarchies made after the call (spmv_amd_mg3d_multi_level_product, lab.h): read here, when a hierarchy
// is made, never on a launch path. The threshold is measured (tools/mg3d_multi_bench.py --products, k = 4): the
// smallest measured grid from which the new kernel is faster with the two ranges apart; 96 and 128 are faster in the median only.
constexpr int kStencil7SpmmMinGrid = 256;
#ifdef SPMV_AMD_LAB
static int g_forced_level_product = 0;  // 0: by the threshold; 1: spmm/csr; 2: spmm/stencil7-row-lds
#endif
static bool stencil7_level_product(int n) {
#ifdef SPMV_AMD_LAB
    if (g_forced_level_product != 0) return g_forced_level_product == 2;
#endif
    return n >= kStencil7SpmmMinGrid;
}

MgMulti* mg_multi_create(const MgHierarchy* h, int max_rhs) {
    MgMulti* mm = new MgMulti();
    mm->max_rhs = max_rhs;
    mm->levels.resize(h->levels.size());
    for (int l = 0; l < h->count(); ++l) {
        const MgLevel& v = h->levels[(size_t)l];
        MgMulti::Level& L = mm->levels[(size_t)l];
        if (v.dim == 3) L.plan = stencil7_level_product(v.n) ? plan_spmm_stencil7(v.view, v.n) : plan_spmm(v.view, Stencil5Variant::Auto, true, v.rows, v.rows);
        else if (v.dim == 0) L.plan = plan_spmm(v.view, Stencil5Variant::Auto, true, v.rows, v.rows);  // an AMG level: "spmm/csr", the operator's own kind
        else L.plan = plan_spmm(v.view, v.plan.variant, false, v.rows, v.rows);
        if (l == 0) continue;
        const size_t count = (size_t)v.rows * (size_t)max_rhs;
        L.R = device_try_alloc<double>(count);
        L.D = device_try_alloc<double>(count);
        L.Z = device_try_alloc<double>(count);
        L.W = device_try_alloc<double>(count);
        if (!L.R || !L.D || !L.Z || !L.W) {
            fprintf(stderr, "[PCG] multigrid: the block vectors of level %d could not be allocated: refused\n", l);
            mg_multi_destroy(mm);
            return nullptr;
        }
    }
    return mm;
}

namespace {

// The batched cycle's operations (mg_schedule.hpp): a level's R, D, Z, W and SpMM plan; level 0 works on the caller's vectors, whose D
// and Z hold term 0 on entry. A launch that carries an SpMM counts as SpMV time, every other as BLAS1.
struct MultiOps {
    struct Vectors {
        const double* R;
        double *D, *Z, *W;
    };
    const MgHierarchy* h;
    const MgMulti* mm;
    int k;
    const PcgMultiColumn* cols;
    Vectors top;
    double* partials;
    long long count;
    StageTimers* T;

    Vectors at(int l) const {
        const MgMulti::Level& M = mm->levels[(size_t)l];
        return l == 0 ? top : Vectors{M.R, M.D, M.Z, M.W};
    }
    void term0(int l) {
        const MgLevel& L = h->levels[(size_t)l];
        const Vectors v = at(l);
        if (l > 0) stage_run(T, &StageTimers::t_blas, [&] { launch_mg_multi_term0(k, L.rows, cols, v.R, L.dinv, L.coef[0], v.D, v.Z); });
    }
    void step(int l, double g, double hh, bool last) {
        const MgLevel& L = h->levels[(size_t)l];
        const Vectors v = at(l);
        stage_run(T, &StageTimers::t_spmv, [&] { launch_spmm(mm->levels[(size_t)l].plan, k, v.Z, v.W, nullptr, kBatchStream); });
        stage_run(T, &StageTimers::t_blas,
                  [&] { launch_pcg_multi_cheb_step(k, L.rows, cols, v.W, v.R, L.dinv, g, hh, v.D, v.Z, last ? 1 : 0, partials, count); });
    }
    void restrict_residual(int l) {
        const MgLevel& L = h->levels[(size_t)l];
        const Vectors v = at(l);
        double* const rc = mm->levels[(size_t)l + 1].R;
        stage_run(T, &StageTimers::t_spmv, [&] {
            if (L.dim == 0) launch_amg_residual_restrict_multi(k, L.view, L.coarse_rows, L.agg_ptr, L.members, cols, v.Z, v.R, rc);
            else if (L.dim == 3) launch_residual_restrict3d_multi(k, L.view, L.n, cols, v.Z, v.R, rc);
            else launch_residual_restrict_multi(k, L.view, cols, v.Z, v.R, rc);
        });
    }
    void prolong(int l) {
        const MgLevel& L = h->levels[(size_t)l];
        stage_run(T, &StageTimers::t_blas, [&] {
            if (L.dim == 0) launch_amg_prolong_correct_multi(k, (size_t)L.rows, L.agg, cols, at(l + 1).Z, at(l).Z);
            else if (L.dim == 3) launch_prolong_correct3d_multi(k, L.n, cols, at(l + 1).Z, at(l).Z);
            else launch_prolong_correct_multi(k, L.n, cols, at(l + 1).Z, at(l).Z);
        });
    }
};

}  // namespace

void mg_cycle_multi(const MgHierarchy* h, int k, const PcgMultiColumn* cols, const double* R, double* D, double* Z, double* W, double* partials,
                    long long count, StageTimers* T) {
    MultiOps ops{h, mg_multi_of(h), k, cols, {R, D, Z, W}, partials, count, T};
    mg_vcycle(ops, h->levels.data(), h->count());
}

}  // namespace spmv_amd

extern "C" int spmv_amd_precond_apply_device_multi(SpmvOperator* op, const SpmvAmdPrecond* m, int nrhs, const double* d_R, double* d_Z) {
    // argument checks: all before the first HIP call
    if (!check_rhs(kTag, nrhs)) return 1;
    if (op == nullptr || m == nullptr || d_R == nullptr || d_Z == nullptr) return fail("apply: null argument"), 1;
    if ((((uintptr_t)d_R) & 15) != 0 || (((uintptr_t)d_Z) & 15) != 0) return fail("apply: a block vector is not 16-byte aligned: refused"), 1;
    const long long n = m->n;
    const int k = nrhs;
    {
        const uintptr_t a = (uintptr_t)d_R, b = (uintptr_t)d_Z, bytes = (uintptr_t)n * k * sizeof(double);
        if (a < b + bytes && b < a + bytes) return fail("apply: d_Z overlaps d_R: refused"), 1;
    }
    const bool mg = m->kind == kMultigrid, cheb = m->kind == kChebyshev, jac = m->kind == kJacobi;
    if (!mg && !cheb && !jac && m->kind != kNone) return fail("apply: unknown preconditioner kind: refused"), 1;
    const int capacity = mg ? mg_multi_capacity(mg_multi_of(m->mg)) : 0;
    if (mg && capacity == 0)
        return fail("apply: kind 'multigrid' keeps single vectors on every level of its hierarchy: not available for several right-hand sides, refused"),
               1;
    if (mg && k > capacity) {
        fprintf(stderr, "[%s] apply: nrhs = %d, the multigrid preconditioner's hierarchy holds block vectors of max_rhs = %d columns: refused\n", kTag,
                k, capacity);
        return 1;
    }
    if (!precond_matches(op, m, diagonal_source_of(op))) return 1;
    MultiOperand o;
    if (cheb || mg) {  // the kinds that run the operator's product
        if (!usable_operator(kTag, op, &o)) return 1;
        if (o.plan.rows != m->n || o.plan.cols != m->n)
            return fail("apply: the operator is not the initialised square one the preconditioner was made from: refused"), 1;
    }

    CgWorkspaceScope scope;
    const size_t count = (size_t)n * k;
    const long long groups = (n + kFlat - 1) / kFlat;
    PcgMultiColumn* cols = nullptr;  // k records of zeros: every column is running
    double *D = nullptr, *W = nullptr, *partials = nullptr;
    bool ok = true;
    if (cheb || mg) {
        char what[64];
        snprintf(what, sizeof what, "an application on %d columns of %lld rows", k, n);
        ok = device_has_room(2 * count * sizeof(double) + ((size_t)64 << 20), kTag, what);
        if (ok) {
            cols = device_try_alloc<PcgMultiColumn>((size_t)k);
            D = device_try_alloc<double>(count);
            W = device_try_alloc<double>(count);
            if (mg) partials = device_try_alloc<double>(2 * (size_t)k * (size_t)groups);  // level 0's last step leaves r.z there
            ok = cols != nullptr && D != nullptr && W != nullptr && (!mg || partials != nullptr);
            if (!ok) fail("apply: the work vectors could not be allocated: refused");
        }
    }
    if (ok) {
        if (cols != nullptr) HIP_CHECK(hipMemsetAsync(cols, 0, (size_t)k * sizeof(PcgMultiColumn), kBatchStream));
        if (mg) {
            launch_mg_multi_term0(k, n, cols, d_R, m->dinv, m->mg->levels[0].coef[0], D, d_Z);
            mg_cycle_multi(m->mg, k, cols, d_R, D, d_Z, W, partials, groups, nullptr);
        } else if (cheb) {
            launch_mg_multi_term0(k, n, cols, d_R, m->dinv, m->coef[0], D, d_Z);
            for (int s = 1; s <= m->degree; ++s) {
                launch_spmm(o.plan, k, d_Z, W, nullptr, kBatchStream);
                launch_pcg_multi_cheb_step(k, n, cols, W, d_R, m->dinv, m->coef[2 * s], m->coef[2 * s - 1], D, d_Z, 0, nullptr, groups);
            }
        } else if (jac) {
            launch_mg_multi_term0(k, n, nullptr, d_R, m->dinv, 1.0, nullptr, d_Z);  // 1.0 * (dinv * r): the bits of dinv * r
        } else {
            HIP_CHECK(hipMemcpyAsync(d_Z, d_R, count * sizeof(double), hipMemcpyDeviceToDevice, kBatchStream));
        }
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
    device_release(cols);
    device_release(D);
    device_release(W);
    device_release(partials);
    return ok ? 0 : 1;
}

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_mg3d_multi_level_product(const char* kind) {
    if (kind != nullptr && !strcmp(kind, "auto")) spmv_amd::g_forced_level_product = 0;
    else if (kind != nullptr && !strcmp(kind, "csr")) spmv_amd::g_forced_level_product = 1;
    else if (kind != nullptr && !strcmp(kind, "stencil7")) spmv_amd::g_forced_level_product = 2;
    else return fail("level product: not one of auto, csr, stencil7: refused"), 1;
    return 0;
}

extern "C" const char* spmv_amd_precond_multigrid_level_spmm(const SpmvAmdPrecond* m, int level) {
    const MgMulti* mm = m != nullptr && m->kind == kMultigrid ? mg_multi_of(m->mg) : nullptr;
    if (mm == nullptr || level < 0 || level >= (int)mm->levels.size()) return "none";
    return mm->levels[(size_t)level].plan.name;
}

static_assert(sizeof(SpmvAmdPcgMultiColumn) == sizeof(PcgMultiColumn), "lab.h's column record is the device record");

// The one body of spmv_amd_mg_multi_stage (dim 2) and spmv_amd_mg_multi_stage3d (dim 3, multigrid3d_multi.hip)
int spmv_amd::mg_multi_stage(int dim, const char* stage, int k, SpmvAmdMgMultiStageArgs* a) {
    // argument checks: all but the structure check before the first HIP call
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    enum Stage { kNoStage, kRestrict, kProlong, kTerm0, kSpmm7, kSpmmCsr } st = kNoStage;
    static const struct {
        const char* name;
        Stage st;
        int dim;
    } kStages[] = {{"residual_restrict", kRestrict, 2},   {"prolong", kProlong, 2},   {"term0", kTerm0, 2},
                   {"residual_restrict3d", kRestrict, 3}, {"prolong3d", kProlong, 3}, {"stencil7_spmm", kSpmm7, 3}, {"spmm_csr", kSpmmCsr, 3}};
    const bool cube = dim == 3;
    if (stage == nullptr)
        return refuse(cube ? "no stage named (residual_restrict3d, prolong3d, stencil7_spmm, spmm_csr)" : "no stage named (residual_restrict, prolong, term0)"), 1;
    for (const auto& known : kStages)
        if (known.dim == dim && !strcmp(stage, known.name)) st = known.st;
    if (st == kNoStage)
        return refuse(cube ? "unknown stage (residual_restrict3d, prolong3d, stencil7_spmm, spmm_csr)" : "unknown stage (residual_restrict, prolong, term0)"), 1;
    const bool product = st == kSpmm7 || st == kSpmmCsr;
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    if (!cube && (a->n < 2 || a->n > 46340)) return refuse("the fine grid is outside 2..46340"), 1;
    if (cube && (a->n < 2 || a->n > kStencil7MaxGrid)) return refuse("the fine grid of a 3-D stage is outside 2..674"), 1;
    const int block = k % 2 == 0 ? 16 : 8;  // a block vector: 16-byte accesses where k is even
    if ((st == kRestrict || product) && (!pointer("row_ptr", a->row_ptr, 4) || !pointer("col_idx", a->col_idx, 4) || !pointer("values", a->values, 8)))
        return 1;
    if (!pointer("z", a->z, block)) return 1;
    if ((st == kRestrict || st == kTerm0) && !pointer("r", a->r, block)) return 1;
    if ((st == kRestrict || st == kProlong) && !pointer("coarse", a->coarse, block)) return 1;
    if ((st == kTerm0 || product) && !pointer("d", a->d, block)) return 1;
    if (st == kTerm0 && !pointer("dinv", a->dinv, 8)) return 1;
    if (a->cols != nullptr && !pointer("cols", a->cols, 8)) return 1;

    const PcgMultiColumn* cols = reinterpret_cast<const PcgMultiColumn*>(a->cols);
    if (st == kRestrict || product) {
        SlabCsr fine = cube ? stencil7_view(a->n, a->row_ptr, a->col_idx, a->values) : mg_stencil_view(a->n, a->row_ptr, a->col_idx, a->values);
        if (cube && !mg_verify_stencil7(fine, a->n)) return refuse("the CSR is not a complete 7-point stencil of that grid"), 1;
        if (!cube && !mg_verify_stencil5(fine)) return refuse("the CSR is not a complete 5-point stencil of that grid"), 1;
        if (st == kSpmm7) launch_spmm(plan_spmm_stencil7(fine, a->n), k, a->z, a->d, nullptr, kBatchStream);
        else if (st == kSpmmCsr) launch_spmm(plan_spmm(fine, Stencil5Variant::Auto, true, fine.n_local, fine.n_local), k, a->z, a->d, nullptr, kBatchStream);
        else if (cube) launch_residual_restrict3d_multi(k, fine, a->n, cols, a->z, a->r, a->coarse);
        else launch_residual_restrict_multi(k, fine, cols, a->z, a->r, a->coarse);
    } else if (st == kProlong) {
        if (cube) launch_prolong_correct3d_multi(k, a->n, cols, a->coarse, a->z);
        else launch_prolong_correct_multi(k, a->n, cols, a->coarse, a->z);
    } else {
        launch_mg_multi_term0(k, (long long)a->n * a->n, cols, a->r, a->dinv, a->c0, a->d, a->z);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

extern "C" int spmv_amd_mg_multi_stage(const char* stage, int k, SpmvAmdMgMultiStageArgs* a) { return mg_multi_stage(2, stage, k, a); }
#endif  // SPMV_AMD_LAB
