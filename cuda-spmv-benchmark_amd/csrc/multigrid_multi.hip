// multigrid_multi.hip -- kind "multigrid" of the batched preconditioned solver (pcg_multi.hip): the V(nu, nu) cycle of multigrid.hip on
// block vectors of up to 8 interleaved columns (multi_rhs.hpp), for the 2-D hierarchy of stencil5-csr (DESIGN.md section 19;
// include/spmv_amd/api.h states the algebra) and, with the restriction and prolongation of multigrid3d_multi.hip in the place of the two
// here, for the 3-D hierarchy of stencil7-csr (spmv_amd_precond_create_multigrid3d_multi). The hierarchy, its coarse operators, dinv, bounds and coefficients are multigrid.hip's;
// spmv_amd_precond_create_multigrid_multi adds what is here: on every level above 0 the block vectors R, D, Z and W of max_rhs columns,
// and on every level an SpmmPlan on the level's own view and Stencil5Plan variant (a 3-D level: "spmm/csr"). Level 0 works on its caller's vectors -- the solve's
// R, D, Z and AP buffer, or the block application's.
//
// A cycle's launch count does not depend on k: the columns share every launch, and the three launches that are multigrid's own read
// what the columns share once --
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

#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "multigrid3d.hpp"
#include "multigrid_device.hpp"
#include "multigrid_multi_device.hpp"
#include "precond.hpp"
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
constexpr int kTileCols = 128;  // fine columns of one residual-restriction tile: lane l owns aggregate column l of the tile
constexpr int kFlat = 256;      // workgroup of the flat kernels
constexpr int kChunk = 4;       // columns one pass of the restriction holds in registers: 12 * 4 doubles of z and r per lane

// any_running, load_run, store_run and the flat walk's FlatWalk, load_unit, store_unit: multigrid_multi_device.hpp

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
__device__ __forceinline__ void restrict_sum(const RestrictRegs<C>& t, const double (*strip)[5 * kTileCols], double* __restrict__ rc, int n,
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
__device__ __forceinline__ void restrict_rest(const double (*strip)[5 * kTileCols], const double* __restrict__ z, const double* __restrict__ r,
                                              double* __restrict__ rc, int n, int nc, int I, int i0, int ja, int lane, bool has_a, bool has_b) {
    if constexpr (C0 < K) {
        constexpr int C = K - C0 < kChunk ? K - C0 : kChunk;
        RestrictRegs<C> next;
        restrict_load<K, C0, C>(next, z, r, n, i0, ja, lane, has_a, has_b);
        restrict_sum<K, C0, C>(next, strip, rc, n, nc, I, ja, lane, has_a, has_b);
        restrict_rest<K, C0 + C>(strip, z, r, rc, n, nc, I, i0, ja, lane, has_a, has_b);
    }
}

// t = fma(-1.0, sum, r) of row (i, j), column q, off the fast path: residual_off_tile of multigrid.hip on interleaved vectors
template <int K>
__device__ __forceinline__ double residual_off_tile_multi(const SlabCsr& m, const double* __restrict__ z, const double* __restrict__ r, int i, int j,
                                                          int q) {
    const int n = m.grid_size;
    const long long row = (long long)i * n + j;
    double sum;
    if (i > 0 && i < n - 1) {
        const double* __restrict__ v = m.values + m.row_ptr[row];
        const double* __restrict__ zl = z + row * K + q;
        const long long up = (long long)n * K;
        if (j > 0 && j < n - 1) sum = stencil5_row(j, n, v[1], zl[-K], v[2], zl[0], v[3], zl[K], v[0], zl[-up], v[4], zl[up]);
        else if (j == 0) sum = stencil5_row(j, n, 0.0, 0.0, v[1], zl[0], v[2], zl[K], v[0], zl[-up], v[3], zl[up]);
        else sum = stencil5_row(j, n, v[1], zl[-K], v[2], zl[0], 0.0, 0.0, v[0], zl[-up], v[3], zl[up]);
    } else {
        sum = 0.0;
        for (int e = m.row_ptr[row]; e < m.row_ptr[row + 1]; ++e) sum = fma(m.values[e], z[(long long)m.col_idx[e] * K + q], sum);
    }
    return fma(-1.0, sum, r[row * K + q]);
}

template <int K>
__global__ __launch_bounds__(kWave) void residual_restrict_multi_kernel(SlabCsr m, const PcgMultiColumn* __restrict__ cols,
                                                                        const double* __restrict__ z, const double* __restrict__ r,
                                                                        double* __restrict__ rc, int nc, int col_tiles, int total_tiles, int run) {
    __shared__ double strip[2][5 * kTileCols];
    if (!any_running<K>(cols)) return;  // uniform over the launch
    const int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    const int n = m.grid_size;
    const int I = tile / col_tiles;
    const int j0 = (tile - I * col_tiles) * kTileCols;
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
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 10; ++s) strip[a][64 * s + lane] = c[a][s];
        wave_lds_sync();
        restrict_sum<K, 0, CA>(first, strip, rc, n, nc, I, ja, lane, has_a, has_b);
        restrict_rest<K, CA>(strip, z, r, rc, n, nc, I, i0, ja, lane, has_a, has_b);
    } else if (has_a) {
        // a pair with grid row 0 or n-1 in it, a lone last grid row
#pragma unroll
        for (int q = 0; q < K; ++q) {
            double acc = residual_off_tile_multi<K>(m, z, r, i0, ja, q);
            if (has_b) acc = acc + residual_off_tile_multi<K>(m, z, r, i0, jb, q);
            if (i1 < n) {
                acc = acc + residual_off_tile_multi<K>(m, z, r, i1, ja, q);
                if (has_b) acc = acc + residual_off_tile_multi<K>(m, z, r, i1, jb, q);
            }
            rc[((long long)I * nc + (ja >> 1)) * K + q] = acc;
        }
    }
}

// ---- the flat kernels: unit f = threadIdx.x + 256 i (i < P) of a workgroup's 256 rows is row f / P, columns (f % P) * V ... + V - 1,
// V = 2 for even K (16-byte accesses), 1 else, P = K / V -- the walk of the batched solvers' vector kernels (multi_rhs_device.hpp) ----
// z[i][j] = fma(2.0, e_c[agg(i)][j], z[i][j]), z in place; the store is plain: the post-smoother's SpMM reads it
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

// ---- the launches: the cycle calls these, and so does the LAB build's spmv_amd_mg_multi_stage ----
int coarse_grid_of(int n) { return (n + 1) / 2; }
unsigned flat_grid(long long rows) { return (unsigned)((rows + kFlat - 1) / kFlat); }

void launch_residual_restrict_multi(int k, const SlabCsr& m, const PcgMultiColumn* cols, const double* z, const double* r, double* rc) {
    const int n = m.grid_size, nc = coarse_grid_of(n);
    const int col_tiles = (n + kTileCols - 1) / kTileCols;
    const int tiles = col_tiles * nc;
    const int run = rowlds_xcd_run_rule(n);
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((residual_restrict_multi_kernel<decltype(K)::value>), dim3((unsigned)xcd_padded_grid(tiles, run)), dim3(kWave), 0,
                           kBatchStream, m, cols, z, r, rc, nc, col_tiles, tiles, run);
    });
}

void launch_prolong_correct_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z) {
    const long long rows = (long long)n * n;
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((prolong_correct_multi_kernel<decltype(K)::value>), dim3(flat_grid(rows)), dim3(kFlat), 0, kBatchStream, rows, n,
                           coarse_grid_of(n), cols, ec, z);
    });
}

void launch_mg_multi_term0(int k, long long rows, const PcgMultiColumn* cols, const double* R, const double* dinv, double c0, double* D, double* Z) {
    dispatch_k(k, [&](auto K) {
        hipLaunchKernelGGL((mg_multi_term0_kernel<decltype(K)::value>), dim3(flat_grid(rows)), dim3(kFlat), 0, kBatchStream, rows, cols, R, dinv, c0,
                           D, Z);
    });
}

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
    for (int l = 1; l < mg_level_count(h); ++l) bytes += 4 * (size_t)mg_level_view(h, l).rows * (size_t)max_rhs * sizeof(double) + 4 * 4096;
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
    mm->levels.resize((size_t)mg_level_count(h));
    for (int l = 0; l < mg_level_count(h); ++l) {
        const MgLevelView v = mg_level_view(h, l);
        MgMulti::Level& L = mm->levels[(size_t)l];
        if (v.dim == 3) L.plan = stencil7_level_product(v.n) ? plan_spmm_stencil7(*v.view, v.n) : plan_spmm(*v.view, Stencil5Variant::Auto, true, v.rows, v.rows);
        else L.plan = plan_spmm(*v.view, v.variant, false, v.rows, v.rows);
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

struct MultiCycle {
    const MgHierarchy* h;
    const MgMulti* mm;
    int k;
    const PcgMultiColumn* cols;
    double* partials;
    long long count;
    StageTimers* T;

    // level l on (R, D, Z, W); D and Z hold term 0 on entry where l == 0
    void level(int l, const double* R, double* D, double* Z, double* W) {
        const MgLevelView v = mg_level_view(h, l);
        const SpmmPlan& plan = mm->levels[(size_t)l].plan;
        const bool coarsest = l + 1 == mg_level_count(h);
        const bool top = l == 0;
        auto step = [&](double g, double hh, bool last) {  // a launch that carries an SpMM counts as SpMV time, every other as BLAS1
            stage_run(T, &StageTimers::t_spmv, [&] { launch_spmm(plan, k, Z, W, nullptr, kBatchStream); });
            stage_run(T, &StageTimers::t_blas,
                      [&] { launch_pcg_multi_cheb_step(k, v.rows, cols, W, R, v.dinv, g, hh, D, Z, last ? 1 : 0, partials, count); });
        };
        if (!top) stage_run(T, &StageTimers::t_blas, [&] { launch_mg_multi_term0(k, v.rows, cols, R, v.dinv, v.coef[0], D, Z); });
        for (int s = 1; s <= v.degree; ++s) step(v.coef[2 * s], v.coef[2 * s - 1], coarsest && top && s == v.degree);  // pre-smoothing / the solve
        if (coarsest) return;
        const MgMulti::Level& C = mm->levels[(size_t)l + 1];
        stage_run(T, &StageTimers::t_spmv, [&] {
            if (v.dim == 3) launch_residual_restrict3d_multi(k, *v.view, v.n, cols, Z, R, C.R);
            else launch_residual_restrict_multi(k, *v.view, cols, Z, R, C.R);
        });
        level(l + 1, C.R, C.D, C.Z, C.W);
        stage_run(T, &StageTimers::t_blas, [&] {
            if (v.dim == 3) launch_prolong_correct3d_multi(k, v.n, cols, C.Z, Z);
            else launch_prolong_correct_multi(k, v.n, cols, C.Z, Z);
        });
        step(v.coef[0], 0.0, top && v.degree == 0);  // post-smoothing from the guess z: term 0 in step form
        for (int s = 1; s <= v.degree; ++s) step(v.coef[2 * s], v.coef[2 * s - 1], top && s == v.degree);
    }
};

}  // namespace

void mg_cycle_multi(const MgHierarchy* h, int k, const PcgMultiColumn* cols, const double* R, double* D, double* Z, double* W, double* partials,
                    long long count, StageTimers* T) {
    MultiCycle run{h, mg_multi_of(h), k, cols, partials, count, T};
    run.level(0, R, D, Z, W);
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
            launch_mg_multi_term0(k, n, cols, d_R, m->dinv, mg_level_view(m->mg, 0).coef[0], D, d_Z);
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

extern "C" int spmv_amd_mg_multi_stage(const char* stage, int k, SpmvAmdMgMultiStageArgs* a) {
    // argument checks: all before the first HIP call
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    enum Stage { kRestrict, kProlong, kTerm0 } st;
    if (stage == nullptr) return refuse("no stage named (residual_restrict, prolong, term0)"), 1;
    if (!strcmp(stage, "residual_restrict")) st = kRestrict;
    else if (!strcmp(stage, "prolong")) st = kProlong;
    else if (!strcmp(stage, "term0")) st = kTerm0;
    else return refuse("unknown stage (residual_restrict, prolong, term0)"), 1;
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    if (a->n < 2 || a->n > 46340) return refuse("the fine grid is outside 2..46340"), 1;
    const int block = k % 2 == 0 ? 16 : 8;  // a block vector: 16-byte accesses where k is even
    if (st == kRestrict && (!pointer("row_ptr", a->row_ptr, 4) || !pointer("col_idx", a->col_idx, 4) || !pointer("values", a->values, 8))) return 1;
    if (!pointer("z", a->z, block)) return 1;
    if (st != kProlong && !pointer("r", a->r, block)) return 1;
    if (st != kTerm0 && !pointer("coarse", a->coarse, block)) return 1;
    if (st == kTerm0 && (!pointer("d", a->d, block) || !pointer("dinv", a->dinv, 8))) return 1;
    if (a->cols != nullptr && !pointer("cols", a->cols, 8)) return 1;

    const PcgMultiColumn* cols = reinterpret_cast<const PcgMultiColumn*>(a->cols);
    if (st == kRestrict) {
        SlabCsr fine = mg_stencil_view(a->n, a->row_ptr, a->col_idx, a->values);
        if (!mg_verify_stencil5(fine)) return refuse("the CSR is not a complete 5-point stencil of that grid"), 1;
        launch_residual_restrict_multi(k, fine, cols, a->z, a->r, a->coarse);
    } else if (st == kProlong) {
        launch_prolong_correct_multi(k, a->n, cols, a->coarse, a->z);
    } else {
        launch_mg_multi_term0(k, (long long)a->n * a->n, cols, a->r, a->dinv, a->c0, a->d, a->z);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}
#endif  // SPMV_AMD_LAB
