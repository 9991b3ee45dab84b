// pcg_multi.hip -- batched preconditioned CG: up to 8 independent systems A x_j = b_j solved together under one preconditioner of
// kind "none", "jacobi" or "chebyshev", one matrix pass per product.
//
// Each column is its own PCG solve -- own alpha, beta, r.z, verdict, history and iteration count, the algebra of
// spmv_amd_pcg_solve_device (pcg.hip, sections 13 and 14) element for element. What the columns share is the SpMM (spmm_kernels.hip),
// which reads the coefficients once for all of them, and one dinv[row] per row. Not block CG: no shared Krylov space.
//
// One iteration on the default stream (block vectors interleaved, multi_rhs.hpp), "none" / "jacobi":
//   AP = A P with the per-column p.Ap partials | sums + step 1 (active = !done, alpha = rz / pAp, an unusable pAp: skip_update) |
//   R -= alpha AP, z = dinv r in registers, the partials of r.r and r.z | sums + step 2 (history, verdict, beta) |
//   X += alpha P, then P = z + beta P unless the column stopped in this iteration
// "chebyshev" of degree K:
//   AP = A P | step 1 | R -= alpha AP with term 0 (D, Z), the r.r partials | step 3 (history, verdict) |
//   K x ( W = A Z into the AP buffer ; the step kernel on the columns still running, the last one leaves the r.z partials ) |
//   step 4 (beta) | X += alpha P, P = Z + beta P
// "multigrid" on a hierarchy with block vectors (spmv_amd_precond_create_multigrid_multi): the Chebyshev shape with
// the rest of a V-cycle (mg_cycle_multi, multigrid_multi.hip) in the place of the K steps -- the r update writes term 0 of level 0 --,
// level 0 on D, Z and the AP buffer; every launch of the cycle tests the column records.
// then one small blocking read of the k column records (the stopping test). A column that converged or broke down is frozen: no
// kernel changes a bit of its X, R, P, D, Z, history or count from the next iteration on. In the iteration in which the last column
// stops the K SpMMs of the Chebyshev steps still run (the step kernels return at once): once per solve, and cheaper than a second
// host read per iteration.
//
// Dot products: the rounded product per row, the workgroup's 256 rows through block_partials (multi_rhs_device.hpp), then the two
// reduction stages of the batched CG solver per value and column -- the same bits for a column whatever k is and whatever slot it
// sits in. A kernel with two values sends them through ONE LDS product array, one after the other (16 KiB at k = 8, so LDS never
// limits the 8 workgroups a CU holds; two arrays would be 32 KiB and 5 workgroups; the price is one more barrier per workgroup).
//
// This file: the kernels, their launchers, the loop, the preconditioner's checks and the LAB build's stage hook. What surrounds the
// loop -- workspace, the other argument checks, upload and download, histories, statistics, print-out -- is multi_solve.hpp, shared
// with cg_multi.hip.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "multi_rhs_device.hpp"
#include "multi_solve.hpp"
#include "multigrid.hpp"
#include "reduce_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr const char* kTag = "PCG-MULTI";

// The kind as the kernels see it: what z is made of decides the loads.
constexpr int kPlain = 0, kJac = 1, kCheb = 2;

// R = b - A x0 (R holds b on entry), z0 = M^-1 r0 as far as one pass goes, the partials of r.r (value 0) and r.z (value 1).
// kPlain / kJac: z = r / dinv r, P = z. kCheb: term 0 in registers -- u = dinv r ; d = c0 u ; z = d -- to D and Z; the r.z partials only
// when term 0 is the whole polynomial (last).
template <int K, int kKind>
__global__ __launch_bounds__(kBlock) void pcg_multi_init_kernel(long long n, const double* __restrict__ AP, const double* __restrict__ dinv,
                                                               double c0, int last, double* __restrict__ R, double* __restrict__ P,
                                                               double* __restrict__ D, double* __restrict__ Z, double* __restrict__ partials,
                                                               long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    __shared__ double prod[kBlock * K];
    double rz[K];
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        double r[V] = {}, z[V] = {};
        if (row0 + t < n) {
            const long long at = (row0 + t) * K + col0;
            double ap[V];
            load_unit_once<V>(AP + at, ap);
            load_unit_once<V>(R + at, r);
            const double dv = kKind == kPlain ? 1.0 : dinv[row0 + t];  // one load per unit: the units of a row read the same 8 bytes
#pragma unroll
            for (int q = 0; q < V; ++q) {
                r[q] = fma(1.0, r[q], -1.0 * ap[q]);
                z[q] = kKind == kPlain ? r[q] : kKind == kJac ? dv * r[q] : c0 * (dv * r[q]);
            }
            store_unit_once<V>(R + at, r);
            if (kKind == kCheb) {
                store_unit_once<V>(D + at, z);
                store_row<V>(Z + at, z);  // plain: the first step's SpMM reads it
            } else {
                store_row<V>(P + at, z);  // plain: the first SpMM reads it
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q], rz[i * V + q] = r[q] * z[q];
    }
    unit_partials<K>(prod, true, rz, kKind != kCheb || last != 0, partials, count);
}

// r = fma(-alpha, Ap, r) for the columns of this iteration whose pAp did not break down; z = M^-1 r as far as one pass goes; the
// partials of r.r (value 0) and r.z (value 1). kPlain / kJac: z stays in the registers. kCheb: term 0 to D and Z for the active
// columns (a frozen column's D and Z keep their bits); the r.z partials only when term 0 is the whole polynomial (last).
template <int K, int kKind>
__global__ __launch_bounds__(kBlock) void pcg_multi_update_r_kernel(long long n, const PcgMultiColumn* __restrict__ cols,
                                                                   const double* __restrict__ AP, const double* __restrict__ dinv, double c0,
                                                                   int last, double* __restrict__ R, double* __restrict__ D,
                                                                   double* __restrict__ Z, double* __restrict__ partials, long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    __shared__ double prod[kBlock * K];
    double rz[K];
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        double r[V] = {}, z[V] = {};
        if (row0 + t < n) {
            const long long at = (row0 + t) * K + col0;
            double ap[V];
            load_unit_once<V>(AP + at, ap);
            load_unit_once<V>(R + at, r);
            const double dv = kKind == kPlain ? 1.0 : dinv[row0 + t];
            bool any = false, all = true;
#pragma unroll
            for (int q = 0; q < V; ++q) {
                const PcgMultiColumn& c = cols[col0 + q];
                if (c.active && !c.skip_update) r[q] = fma(-c.alpha, ap[q], r[q]);
                z[q] = kKind == kPlain ? r[q] : kKind == kJac ? dv * r[q] : c0 * (dv * r[q]);
                any = any || c.active, all = all && c.active;
            }
            store_unit_once<V>(R + at, r);
            if (kKind == kCheb && any) {
                double dz[V], zz[V];
#pragma unroll
                for (int q = 0; q < V; ++q) dz[q] = zz[q] = z[q];
                if (!all) {  // a frozen column beside an active one in a 16-byte pair: its bits go back as they came
                    double dk[V], zk[V];
                    load_row<V>(D + at, dk);
                    load_row<V>(Z + at, zk);
#pragma unroll
                    for (int q = 0; q < V; ++q)
                        if (!cols[col0 + q].active) dz[q] = dk[q], zz[q] = zk[q];
                }
                store_unit_once<V>(D + at, dz);
                store_row<V>(Z + at, zz);  // plain: the first step's SpMM reads it
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q], rz[i * V + q] = r[q] * z[q];
    }
    unit_partials<K>(prod, true, rz, kKind != kCheb || last != 0, partials, count);
}

// One Chebyshev step behind a SpMM that wrote W = A Z, on the columns still running (done == 0):
// d = fma(g, dinv * fma(-1, w, r), h * d) ; z = z + d, D and Z in place. last: the partials of r.z as value 1 (value 0, r.r, stays
// as the r update left it). Nothing is read for a unit without a running column, and nothing at all once every column is done.
template <int K>
__global__ __launch_bounds__(kBlock) void pcg_multi_cheb_step_kernel(long long n, const PcgMultiColumn* __restrict__ cols,
                                                                    const double* __restrict__ W, const double* __restrict__ R,
                                                                    const double* __restrict__ dinv, double g, double h, double* __restrict__ D,
                                                                    double* __restrict__ Z, int last, double* __restrict__ partials,
                                                                    long long count) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    __shared__ double prod[kBlock * K];
    bool running = false;
#pragma unroll
    for (int j = 0; j < K; ++j) running = running || cols[j].done == 0;
    if (!running) return;  // uniform over the launch
    double rz[K];
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        bool run[V], any = false;
#pragma unroll
        for (int q = 0; q < V; ++q) run[q] = cols[col0 + q].done == 0, any = any || run[q], rz[i * V + q] = 0.0;
        if (any && row0 + t < n) {
            const long long at = (row0 + t) * K + col0;
            double w[V], r[V], d[V], z[V];
            load_unit_once<V>(W + at, w);
            load_unit_once<V>(R + at, r);
            load_unit_once<V>(D + at, d);
            load_row<V>(Z + at, z);
            const double dv = dinv[row0 + t];
#pragma unroll
            for (int q = 0; q < V; ++q) {
                if (!run[q]) continue;
                d[q] = fma(g, dv * fma(-1.0, w[q], r[q]), h * d[q]);
                z[q] = z[q] + d[q];
                rz[i * V + q] = r[q] * z[q];
            }
            store_unit_once<V>(D + at, d);
            store_row<V>(Z + at, z);  // plain: the next SpMM reads it
        }
    }
    if (last) unit_partials<K>(prod, false, rz, true, partials, count);
}

// x = fma(alpha, p, x) for the columns of this iteration whose pAp did not break down; then p = fma(beta, p, z) for those that did
// not stop in it. z: dinv r (kJac), r (kPlain) from ZR = R, or ZR = Z (kCheb). Nothing is read for a unit without such a column.
template <int K, int kKind>
__global__ __launch_bounds__(kBlock) void pcg_multi_update_xp_kernel(long long n, const PcgMultiColumn* __restrict__ cols,
                                                                    const double* __restrict__ ZR, const double* __restrict__ dinv,
                                                                    double* __restrict__ P, double* __restrict__ X) {
    constexpr int V = Flat<K>::V, U = Flat<K>::P;
    const long long row0 = (long long)blockIdx.x * kBlock;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int f = (int)threadIdx.x + kBlock * i;
        const int t = f / U, col0 = (f - t * U) * V;
        if (row0 + t >= n) continue;
        bool upd[V], dir[V], any_upd = false, any_dir = false;
        double alpha[V], beta[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const PcgMultiColumn& c = cols[col0 + q];
            upd[q] = c.active != 0 && c.skip_update == 0;
            dir[q] = upd[q] && c.done == 0;
            alpha[q] = c.alpha, beta[q] = c.beta;
            any_upd = any_upd || upd[q], any_dir = any_dir || dir[q];
        }
        if (!any_upd) continue;
        const long long at = (row0 + t) * K + col0;
        double x[V], p[V], z[V] = {};
        double dv = 1.0;
        load_unit_once<V>(X + at, x);  // every load of the unit before the first use: one wait, not two
        load_unit_once<V>(P + at, p);
        if (any_dir) {
            load_unit_once<V>(ZR + at, z);
            if (kKind == kJac) dv = dinv[row0 + t];
        }
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (upd[q]) x[q] = fma(alpha[q], p[q], x[q]);
        store_unit_once<V>(X + at, x);
        if (!any_dir) continue;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            if (kKind == kJac) z[q] = dv * z[q];
            if (dir[q]) p[q] = fma(beta[q], p[q], z[q]);
        }
        store_row<V>(P + at, p);  // plain: the next SpMM's neighbour loads re-use these lines
    }
}

// pcg.hip's pcg_step, per column and branch for branch. which: 0 = initial r.r / r.z, 1 = pAp, 2 = r.r / r.z', 3 = r.r and the verdict
// alone, 4 = r.z' and beta alone (the last two: kind "chebyshev").
__device__ void pcg_multi_step(PcgMultiColumn& c, int which, const double* total, double tol, double* hist, int hist_cap) {
    if (which == 0) {
        c.b_norm = sqrt(total[0]);
        c.residual = c.b_norm;
        c.rz = total[1];
        c.pAp = c.alpha = c.beta = 0.0;
        c.active = c.done = c.iterations = c.converged = c.breakdown = c.skip_update = 0;
        if (hist_cap > 0) hist[0] = c.b_norm;
    } else if (which == 1) {
        c.active = c.done ? 0 : 1;
        if (!c.active) return;
        c.pAp = total[0];
        if (usable(c.pAp)) {
            c.alpha = c.rz / c.pAp;
        } else {
            c.alpha = 0.0;
            c.skip_update = 1;
        }
    } else if (!c.active) {
        return;
    } else if (which == 2 || which == 3) {
        const double res = sqrt(total[0]);
        c.iterations += 1;
        c.residual = res;
        if (c.iterations < hist_cap) hist[c.iterations] = res;
        if (c.skip_update) {
            c.breakdown = 1;
        } else if (res / c.b_norm < tol) {
            c.converged = 1;
        } else if (which == 2) {
            if (!usable(total[1])) {
                c.breakdown = 1;
            } else {
                c.beta = total[1] / c.rz;
                c.rz = total[1];
            }
        }
        c.done = (c.converged != 0 || c.breakdown != 0) ? 1 : 0;
    } else if (c.done == 0) {  // which == 4
        if (!usable(total[0])) {
            c.breakdown = 1;
            c.done = 1;
        } else {
            c.beta = total[0] / c.rz;
            c.rz = total[0];
        }
    }
}

// Stage 2 of each value + the scalar step of column j (workgroup j). Value v of column j: slices[(v * k + j) * slice_count ...].
__global__ __launch_bounds__(kBlock) void pcg_multi_step_kernel(const double* __restrict__ slices, int slice_count, int k, int nv, int which,
                                                               double tol, PcgMultiColumn* __restrict__ cols, double* __restrict__ hist,
                                                               int hist_cap) {
    __shared__ double s[kBlock];
    const int j = (int)blockIdx.x;
    double total[2] = {0.0, 0.0};
    for (int v = 0; v < nv; ++v) {
        const double* __restrict__ src = slices + ((long long)v * k + j) * slice_count;
        double acc = 0.0;
        for (int i = (int)threadIdx.x; i < slice_count; i += kBlock) acc += src[i];
        block_tree(acc, s);
        total[v] = s[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) pcg_multi_step(cols[j], which, total, tol, hist + (long long)j * hist_cap, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_pcg_multi_stage ----

struct VecArgs {
    long long n;
    const PcgMultiColumn* cols;
    const double* dinv;
    double c0, g, h;  // c0: term 0; g, h: one Chebyshev step
    int last;
    double *X, *R, *P, *AP, *D, *Z;
    double* partials;
    long long count;
};
enum { kStageInit, kStageUpdateR, kStageUpdateXp, kStageChebStep };

template <int K, int kKind>
void launch_vec_kind(int stage, const VecArgs& a) {
    const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock)), block(kBlock);
    if (stage == kStageInit)
        hipLaunchKernelGGL((pcg_multi_init_kernel<K, kKind>), grid, block, 0, kBatchStream, a.n, a.AP, a.dinv, a.c0, a.last, a.R, a.P, a.D, a.Z,
                           a.partials, a.count);
    else if (stage == kStageUpdateR)
        hipLaunchKernelGGL((pcg_multi_update_r_kernel<K, kKind>), grid, block, 0, kBatchStream, a.n, a.cols, a.AP, a.dinv, a.c0, a.last, a.R, a.D, a.Z,
                           a.partials, a.count);
    else
        hipLaunchKernelGGL((pcg_multi_update_xp_kernel<K, kKind>), grid, block, 0, kBatchStream, a.n, a.cols, kKind == kCheb ? a.Z : a.R, a.dinv, a.P,
                           a.X);
}

template <int K>
void launch_vec(int stage, int kind, const VecArgs& a) {
    if (stage == kStageChebStep) {
        const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock)), block(kBlock);
        hipLaunchKernelGGL((pcg_multi_cheb_step_kernel<K>), grid, block, 0, kBatchStream, a.n, a.cols, a.AP, a.R, a.dinv, a.g, a.h, a.D, a.Z, a.last,
                           a.partials, a.count);
    } else if (kind == kCheb) {
        launch_vec_kind<K, kCheb>(stage, a);
    } else if (kind == kJac) {
        launch_vec_kind<K, kJac>(stage, a);
    } else {
        launch_vec_kind<K, kPlain>(stage, a);
    }
}

// kind: kPlain, kJac, kCheb. a.count = the workgroups of the launch.
void launch_vector_stage(int k, int stage, int kind, const VecArgs& a) {
    auto launch = [&](auto K) { launch_vec<decltype(K)::value>(stage, kind, a); };
    if (!dispatch_k(k, launch)) launch(std::integral_constant<int, kMaxRhs>{});
}

int values_of_step(int which) { return which == 0 || which == 2 ? 2 : 1; }

// The two reduction launches behind a scalar step: nv x k x slices_for(count) slice sums of the values at `partials` (value v of
// column j at [(v * k + j) * count ...]), then per column their sums and step `which`. slices: 2 k x slices_for(count) doubles.
void launch_reduce(int k, const double* partials, long long count, double* slices, int which, double tol, PcgMultiColumn* cols, double* hist,
                   int hist_cap) {
    const int sc = slices_for(count), nv = values_of_step(which);
    hipLaunchKernelGGL(multi_reduce_slices_kernel, dim3((unsigned)sc, (unsigned)(nv * k)), dim3(kBlock), 0, kBatchStream, partials, count, sc, slices);
    hipLaunchKernelGGL(pcg_multi_step_kernel, dim3((unsigned)k), dim3(kBlock), 0, kBatchStream, slices, sc, k, nv, which, tol, cols, hist, hist_cap);
}

BatchedWorkspace<PcgMultiColumn> g_ws(2);    // two dot-product values per launch: r.r and r.z
std::vector<std::vector<double>> g_history;  // of the last batched preconditioned solve, per column

ColumnSummary summary_of(const PcgMultiColumn& c) {
    return {c.iterations, c.converged != 0, c.breakdown != 0, c.residual, c.b_norm, c.active != 0};
}

bool fail(const char* what) { return batched_fail(kTag, what); }

}  // namespace

namespace spmv_amd {
void launch_pcg_multi_cheb_step(int k, long long n, const PcgMultiColumn* cols, const double* W, const double* R, const double* dinv, double g,
                                double h, double* D, double* Z, int last, double* partials, long long count) {
    VecArgs a{};
    a.n = n, a.cols = cols, a.dinv = dinv, a.g = g, a.h = h, a.last = last;
    a.AP = const_cast<double*>(W), a.R = const_cast<double*>(R), a.D = D, a.Z = Z, a.partials = partials, a.count = count;
    launch_vector_stage(k, kStageChebStep, kCheb, a);
}
void release_pcg_multi_workspace_locked() { g_ws.release(); }
size_t pcg_multi_workspace_bytes_locked() { return g_ws.bytes(); }
}  // namespace spmv_amd

extern "C" int spmv_amd_pcg_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int nrhs, const double* B, double* X,
                                               const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (op == nullptr || m == nullptr) return fail("null argument"), 1;  // the two pointers the shared checks do not name so
    MultiOperand o;
    if (!check_batched_system(kTag, kTag, op, mat, nrhs, B, X, config, stats, &o)) return 1;
    // kind "multigrid": a hierarchy with block vectors (spmv_amd_precond_create_multigrid_multi) of at least nrhs columns
    const bool mg = m->kind == kMultigrid;
    const int capacity = mg ? mg_multi_capacity(mg_multi_of(m->mg)) : 0;
    if (mg && capacity == 0)
        return fail("kind 'multigrid' keeps single vectors on every level of its hierarchy: not available for several right-hand sides, refused"), 1;
    if (mg && nrhs > capacity) {
        fprintf(stderr, "[%s] nrhs = %d, the multigrid preconditioner's hierarchy holds block vectors of max_rhs = %d columns: refused\n", kTag, nrhs,
                capacity);
        return 1;
    }
    if (!mg && m->kind != kNone && m->kind != kJacobi && m->kind != kChebyshev) return fail("unknown preconditioner kind: refused"), 1;
    if (m->n != mat->rows) {
        fprintf(stderr, "[%s] the preconditioner is for %d rows, mat->rows = %d\n", kTag, m->n, mat->rows);
        return 1;
    }
    if (!precond_matches(op, m, diagonal_source_of(op))) return fail("the preconditioner does not belong to this operator as it stands: refused"), 1;
    const int n = mat->rows, k = nrhs;
    const CGConfig cfg = *config;
    // the kernels' kind: a multigrid cycle begins with term 0 of level 0, so its init and r update are the Chebyshev ones
    const int kind = (m->kind == kChebyshev || mg) ? kCheb : m->kind == kJacobi ? kJac : kPlain;
    const int degree = m->kind == kChebyshev ? m->degree : 0;
    const double c0 = mg ? m->mg->levels[0].coef[0] : m->kind == kChebyshev ? m->coef[0] : 0.0;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const long long vec_count = ((long long)n + kBlock - 1) / kBlock;
    const long long spmm_count = o.plan.blocks;
    BatchedWorkspace<PcgMultiColumn>& w = g_ws;
    if (!w.ensure(kTag, n, k, device, vec_count > spmm_count ? vec_count : spmm_count, cfg.max_iters + 1, kind == kCheb)) return 1;
    load_block_system(w, k, n, B, X, true);  // the records as zeros: done = 0, so the first application's steps run

    std::vector<ColumnSummary> cols;
    StageTimers T(cfg.enable_detailed_timers != 0, kBatchStream);
    VecArgs a{};
    a.n = n, a.cols = w.cols, a.dinv = m->dinv, a.c0 = c0, a.last = (degree == 0 && !mg) ? 1 : 0;  // a cycle never ends with term 0
    a.X = w.X, a.R = w.R, a.P = w.P, a.AP = w.AP, a.D = w.D, a.Z = w.Z, a.partials = w.partials, a.count = vec_count;
    auto vec = [&](int stage) { T.run(&T.t_blas, [&] { launch_vector_stage(k, stage, kind, a); }); };
    auto reduce = [&](const double* partials, long long count, int which) {
        T.run(&T.t_red, [&] { launch_reduce(k, partials, count, w.slices, which, cfg.tolerance, w.cols, w.hist, w.hist_cap); });
    };
    auto spmm = [&](const double* in, double* partials) { T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, in, w.AP, partials, kBatchStream); }); };
    // What follows a term 0 that left D and Z. "chebyshev": steps 1 .. degree, W = A Z goes to the AP buffer, free between the r update
    // and the next SpMM. "multigrid" (degree is 0 here): the rest of the V-cycle, level 0 on D, Z and the AP buffer; every launch of it
    // tests the column records.
    auto after_term0 = [&] {
        if (mg) mg_cycle_multi(m->mg, k, w.cols, w.R, w.D, w.Z, w.AP, w.partials, vec_count, &T);
        for (int s = 1; s <= degree; ++s) {
            spmm(w.Z, nullptr);
            VecArgs c = a;
            c.g = m->coef[2 * s], c.h = m->coef[2 * s - 1], c.last = s == degree ? 1 : 0;
            T.run(&T.t_blas, [&] { launch_vector_stage(k, kStageChebStep, kind, c); });
        }
    };

    T.total.begin(kBatchStream);
    spmm(w.X, nullptr);
    vec(kStageInit);
    if (kind == kCheb) {
        after_term0();
        HIP_CHECK(hipMemcpyAsync(w.P, w.Z, (size_t)n * k * sizeof(double), hipMemcpyDeviceToDevice, kBatchStream));  // p0 = z0
    }
    reduce(w.partials, vec_count, 0);
    read_columns(w, k, summary_of, cols);
    if (cfg.verbose >= 1) print_initial_residuals(kTag, cols, spmv_amd_precond_kind(m));
    for (int it = 0; it < cfg.max_iters && any_column_running(cols); ++it) {
        spmm(w.P, w.partials);
        reduce(w.partials, spmm_count, 1);
        vec(kStageUpdateR);
        if (kind == kCheb) {
            reduce(w.partials, vec_count, 3);
            after_term0();
            reduce(w.partials + (size_t)k * vec_count, vec_count, 4);
        } else {
            reduce(w.partials, vec_count, 2);
        }
        vec(kStageUpdateXp);
        read_columns(w, k, summary_of, cols);  // synchronises: the stopping test of every column
        if (cfg.verbose >= 2) print_iteration(kTag, cols);
    }
    T.total.end(kBatchStream);
    finish_batched_solve(kTag, w, k, n, X, stats, cfg, T, T.total.elapsed_ms(), cols, g_history);
    return 0;
}

extern "C" size_t spmv_amd_pcg_multi_workspace_bytes(void) {
    CgWorkspaceScope scope;
    return pcg_multi_workspace_bytes_locked();
}

extern "C" int spmv_amd_pcg_last_history_multi(int rhs, double* out, int cap) {
    if (rhs < 0 || rhs >= (int)g_history.size()) return -1;
    return copy_history(g_history[(size_t)rhs], out, cap);
}

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_pcg_multi_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdPcgMultiColumn) == sizeof(PcgMultiColumn) && offsetof(SpmvAmdPcgMultiColumn, rz) == offsetof(PcgMultiColumn, rz) &&
                  offsetof(SpmvAmdPcgMultiColumn, pAp) == offsetof(PcgMultiColumn, pAp) &&
                  offsetof(SpmvAmdPcgMultiColumn, alpha) == offsetof(PcgMultiColumn, alpha) &&
                  offsetof(SpmvAmdPcgMultiColumn, beta) == offsetof(PcgMultiColumn, beta) &&
                  offsetof(SpmvAmdPcgMultiColumn, b_norm) == offsetof(PcgMultiColumn, b_norm) &&
                  offsetof(SpmvAmdPcgMultiColumn, residual) == offsetof(PcgMultiColumn, residual) &&
                  offsetof(SpmvAmdPcgMultiColumn, active) == offsetof(PcgMultiColumn, active) &&
                  offsetof(SpmvAmdPcgMultiColumn, done) == offsetof(PcgMultiColumn, done) &&
                  offsetof(SpmvAmdPcgMultiColumn, iterations) == offsetof(PcgMultiColumn, iterations) &&
                  offsetof(SpmvAmdPcgMultiColumn, converged) == offsetof(PcgMultiColumn, converged) &&
                  offsetof(SpmvAmdPcgMultiColumn, breakdown) == offsetof(PcgMultiColumn, breakdown) &&
                  offsetof(SpmvAmdPcgMultiColumn, skip_update) == offsetof(PcgMultiColumn, skip_update),
              "lab.h's column record is the device record, field for field");


extern "C" int spmv_amd_pcg_multi_stage(const char* stage, const char* kind, int k, SpmvAmdPcgMultiStageArgs* a) {
    // argument checks: all before the first HIP call. 16: a block vector the vector kernels access in 16-byte pairs
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    int st;
    if (stage == nullptr) return refuse("no stage named (init, update_r, update_xp, cheb_step, reduce)"), 1;
    if (!strcmp(stage, "init")) st = kStageInit;
    else if (!strcmp(stage, "update_r")) st = kStageUpdateR;
    else if (!strcmp(stage, "update_xp")) st = kStageUpdateXp;
    else if (!strcmp(stage, "cheb_step")) st = kStageChebStep;
    else if (!strcmp(stage, "reduce")) st = -1;
    else return refuse("unknown stage (init, update_r, update_xp, cheb_step, reduce)"), 1;
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    int kd = kPlain;
    if (st == -1) {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 4) return refuse("which is not 0 to 4"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (!pointer("partials", a->partials, 8) || !pointer("cols", a->cols, 8)) return 1;
        if (a->hist_cap > 0 && !pointer("hist", a->hist, 8)) return 1;
    } else {
        if (kind == nullptr) return refuse("no preconditioner kind named (none, jacobi, chebyshev)"), 1;
        if (!strcmp(kind, "none")) kd = kPlain;
        else if (!strcmp(kind, "jacobi")) kd = kJac;
        else if (!strcmp(kind, "chebyshev")) kd = kCheb;
        else return refuse("unknown preconditioner kind (none, jacobi, chebyshev)"), 1;
        if (st == kStageChebStep && kd != kCheb) return refuse("the stage belongs to kind chebyshev"), 1;
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
        if (kd != kPlain && !pointer("dinv", a->dinv, 8)) return 1;
        if (st != kStageInit && !pointer("cols", a->cols, 8)) return 1;
        if (st != kStageUpdateXp && (!pointer("AP", a->AP, 16) || !pointer("partials", a->partials, 8))) return 1;
        if ((st != kStageUpdateXp || kd != kCheb) && !pointer("R", a->R, 16)) return 1;
        if ((st == kStageUpdateXp || (st == kStageInit && kd != kCheb)) && !pointer("P", a->P, 16)) return 1;
        if (st == kStageUpdateXp && !pointer("X", a->X, 16)) return 1;
        if (kd == kCheb && !pointer("Z", a->Z, 16)) return 1;
        if (kd == kCheb && st != kStageUpdateXp && !pointer("D", a->D, 16)) return 1;
    }

    PcgMultiColumn* cols = reinterpret_cast<PcgMultiColumn*>(a->cols);
    double* slices = nullptr;
    if (st == -1) {
        slices = device_alloc<double>(2 * (size_t)k * slices_for(a->count));
        launch_reduce(k, a->partials, a->count, slices, a->which, a->tol, cols, a->hist, a->hist_cap);
    } else {
        VecArgs v{};
        v.n = (long long)a->n, v.cols = cols, v.dinv = a->dinv, v.c0 = a->c0, v.g = a->g, v.h = a->h, v.last = a->last;
        v.X = a->X, v.R = a->R, v.P = a->P, v.AP = a->AP, v.D = a->D, v.Z = a->Z, v.partials = a->partials;
        v.count = (v.n + kBlock - 1) / kBlock;
        launch_vector_stage(k, st, kd, v);
        a->count = v.count;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    device_release(slices);
    return 0;
}
#endif  // SPMV_AMD_LAB