// bicgstab_multi.hip -- batched BiCGSTAB: up to 8 independent nonsymmetric systems A x_j = b_j solved together under one
// preconditioner of kind "none" or "jacobi", one matrix pass per product.
//
// Each column is its own BiCGSTAB solve -- own rho, alpha, omega, beta, verdict, history and iteration count, the algebra of
// spmv_amd_bicgstab_solve_device (bicgstab.hip, steps 1-7 of its header, bicg_step branch for branch) element for element. What the
// columns share is the SpMM (spmm_kernels.hip), which reads the coefficients once for all of them, and one dinv[row] per row. Not a
// block Krylov method: no shared space.
//
// One iteration on the default stream (block vectors interleaved, multi_rhs.hpp; a hat means "times dinv", kind "none": the same
// buffer -- P^ is P, S^ is R):
//   V = A P^ | the partials of r^0.v | sums + step 1 (active = !done, alpha = rho / sigma or the sigma verdict) |
//   the s kernel: R -= alpha V in place on the running columns (R holds s from here to the x / r kernel), "jacobi": S^ = dinv s, the
//   partials of s.s | sums + step 2 (the half step's verdict) | T = A S^ (all columns; stopped ones ignore it) |
//   the partials of t.s and t.t | sums + step 3 (omega or its verdict) | the x / r kernel, per column by its x_step, with the partials
//   of r.r and r^0.r | sums + step 4 (record, stopping test, rho', beta) | the direction kernel: P and P^
// then one small blocking read of the k column records. A column is RUNNING behind step 1 when it is active and not done; a column
// that stopped in this iteration (active and done) still gets from the x / r kernel exactly what the single solver applies (x_step 0,
// 1 or 2). A column that has converged or broken down is frozen: from the next iteration on no kernel changes a bit of its X, R, r^0,
// P, P^, history, count or record; V, T and S^ are scratch for stopped columns (T = A S^ is computed for them and never read). A NaN
// or inf of one column stays in that column.
//
// Dot products: pcg_multi.hip's shape -- the rounded product per row, the workgroup's 256 rows through block_partials
// (multi_rhs_device.hpp), then the two reduction stages per value and column -- so a column has the same bits whatever k is and
// whatever slot it sits in (not the bits of the single-RHS solver, whose dots are streaming fma chains). A column a kernel does not
// work on contributes products of 0.0: its partials never depend on its data.
//
// Vector kernels: templated on K = 1..8, the Flat<K> walk (16-byte accesses for even k), every load of a unit before the first use,
// nontemporal loads and stores for streams touched once per pass, plain stores for what the next SpMM reads. A unit without a column
// that needs it reads nothing; a launch without such a column returns at once; a frozen column beside a running one in a 16-byte pair
// gets its bits back as they came.
//
// This file: the kernels, their launchers, the workspace, the loop and the LAB build's stage hook. What surrounds the loop is
// multi_solve.hpp, shared with cg_multi.hip and pcg_multi.hip.
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
#include "precond.hpp"
#include "reduce_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr const char* kTag = "BICGSTAB-MULTI";

__device__ __forceinline__ bool running(const BicgMultiColumn& c) { return c.active != 0 && c.done == 0; }

// The walk of one workgroup: unit i of this thread is row t of the workgroup, columns col0 .. col0 + V - 1.
#define BICG_MULTI_UNITS                                    \
    constexpr int V = Flat<K>::V, U = Flat<K>::P;           \
    const long long row0 = (long long)blockIdx.x * kBlock;  \
    _Pragma("unroll") for (int i = 0; i < U; ++i)
#define BICG_MULTI_UNIT                       \
    const int f = (int)threadIdx.x + kBlock * i; \
    const int t = f / U, col0 = (f - t * U) * V; \
    const long long at = (row0 + t) * K + col0;  \
    const bool inside = row0 + t < n

// R = fma(1.0, b, -1.0 * A x0) (R holds b on entry) ; r^0 = r ; p = r ; p^ = dinv p ; the partials of r.r
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void bicg_multi_init_kernel(long long n, const double* __restrict__ AX, const double* __restrict__ dinv,
                                                                double* __restrict__ R, double* __restrict__ RH, double* __restrict__ P,
                                                                double* __restrict__ PH, double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    double unused[K] = {};
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        double r[V] = {};
        if (inside) {
            double ax[V];
            load_unit_once<V>(AX + at, ax);
            load_unit_once<V>(R + at, r);
            const double dv = kJac ? dinv[row0 + t] : 1.0;  // one load per unit: the units of a row read the same 8 bytes
#pragma unroll
            for (int q = 0; q < V; ++q) r[q] = fma(1.0, r[q], -1.0 * ax[q]);
            store_unit_once<V>(R + at, r);
            store_unit_once<V>(RH + at, r);
            if (kJac) {
                double h[V];
#pragma unroll
                for (int q = 0; q < V; ++q) h[q] = dv * r[q];
                store_unit_once<V>(P + at, r);
                store_row<V>(PH + at, h);  // plain: the first SpMM reads it
            } else {
                store_row<V>(P + at, r);
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q];
    }
    unit_partials<K>(prod, true, unused, false, partials, count);
}

// The partials of r^0.v for the columns that are not done (step 1, which sets `active`, comes behind this launch).
template <int K>
__global__ __launch_bounds__(kBlock) void bicg_multi_dot_rv_kernel(long long n, const BicgMultiColumn* __restrict__ cols,
                                                                  const double* __restrict__ RH, const double* __restrict__ VV,
                                                                  double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    bool need = false;
#pragma unroll
    for (int j = 0; j < K; ++j) need = need || cols[j].done == 0;
    if (!need) return;  // uniform over the launch
    double unused[K] = {};
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        bool run[V], any = false;
#pragma unroll
        for (int q = 0; q < V; ++q) run[q] = cols[col0 + q].done == 0, any = any || run[q];
        double h[V] = {}, v[V] = {};
        if (any && inside) {
            load_unit_once<V>(RH + at, h);
            load_unit_once<V>(VV + at, v);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = run[q] ? h[q] * v[q] : 0.0;
    }
    unit_partials<K>(prod, true, unused, false, partials, count);
}

// The running columns: s = fma(-alpha, v, r) in place (R holds s from here to the x / r kernel) ; s^ = dinv s ; the partials of s.s
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void bicg_multi_update_s_kernel(long long n, const BicgMultiColumn* __restrict__ cols,
                                                                    const double* __restrict__ VV, const double* __restrict__ dinv,
                                                                    double* __restrict__ R, double* __restrict__ SH,
                                                                    double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    bool need = false;
#pragma unroll
    for (int j = 0; j < K; ++j) need = need || running(cols[j]);
    if (!need) return;  // uniform over the launch
    double unused[K] = {};
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        bool run[V], any = false, all = true;
        double alpha[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const BicgMultiColumn& c = cols[col0 + q];
            run[q] = running(c), alpha[q] = c.alpha;
            any = any || run[q], all = all && run[q];
        }
        double r[V] = {};
        if (any && inside) {
            double v[V], keep[V] = {};
            load_unit_once<V>(VV + at, v);
            load_unit_once<V>(R + at, r);
            const double dv = kJac ? dinv[row0 + t] : 1.0;
            if (kJac && !all) load_row<V>(SH + at, keep);  // a stopped column beside a running one: its bits go back as they came
#pragma unroll
            for (int q = 0; q < V; ++q)
                if (run[q]) r[q] = fma(-alpha[q], v[q], r[q]);
            if (kJac) {
                double h[V];
#pragma unroll
                for (int q = 0; q < V; ++q) h[q] = run[q] ? dv * r[q] : keep[q];
                store_unit_once<V>(R + at, r);
                store_row<V>(SH + at, h);  // plain: the second SpMM reads it
            } else {
                store_row<V>(R + at, r);  // plain: s^ is s, the second SpMM reads it
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = run[q] ? r[q] * r[q] : 0.0;
    }
    unit_partials<K>(prod, true, unused, false, partials, count);
}

// The running columns: the partials of t.s (value 0) and t.t (value 1), s read from R.
template <int K>
__global__ __launch_bounds__(kBlock) void bicg_multi_dot_t_kernel(long long n, const BicgMultiColumn* __restrict__ cols,
                                                                 const double* __restrict__ TT, const double* __restrict__ R,
                                                                 double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    bool need = false;
#pragma unroll
    for (int j = 0; j < K; ++j) need = need || running(cols[j]);
    if (!need) return;  // uniform over the launch
    double tt[K];
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        bool run[V], any = false;
#pragma unroll
        for (int q = 0; q < V; ++q) run[q] = running(cols[col0 + q]), any = any || run[q];
        double tv[V] = {}, s[V] = {};
        if (any && inside) {
            load_unit_once<V>(TT + at, tv);
            load_unit_once<V>(R + at, s);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            prod[t * K + col0 + q] = run[q] ? tv[q] * s[q] : 0.0;
            tt[i * V + q] = run[q] ? tv[q] * tv[q] : 0.0;
        }
    }
    unit_partials<K>(prod, true, tt, true, partials, count);
}

// Per active column by its x_step -- 2: x = fma(omega, s^, fma(alpha, p^, x)) ; r = fma(-omega, t, s) in place ; the partials of r.r
// (value 0) and r^0.r (value 1). 1 (half step, omega breakdown): x = fma(alpha, p^, x) alone, R keeps s. 0 (sigma breakdown, or a
// column that was frozen before this iteration): nothing. kind "none": PH is P and s^ is s.
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void bicg_multi_update_xr_kernel(long long n, const BicgMultiColumn* __restrict__ cols,
                                                                     const double* __restrict__ PH, const double* __restrict__ SH,
                                                                     const double* __restrict__ TT, const double* __restrict__ RH,
                                                                     double* __restrict__ X, double* __restrict__ R,
                                                                     double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    bool need = false;
#pragma unroll
    for (int j = 0; j < K; ++j) need = need || cols[j].active != 0;
    if (!need) return;  // uniform over the launch
    double hr[K];
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        int step[V];
        bool any = false, whole = false;
        double alpha[V], omega[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const BicgMultiColumn& c = cols[col0 + q];
            step[q] = c.active != 0 ? c.x_step : 0;
            alpha[q] = c.alpha, omega[q] = c.omega;
            any = any || step[q] != 0, whole = whole || step[q] == 2;
        }
        double rr[V] = {}, hh[V] = {};
        if (any && inside) {
            double x[V], p[V], s[V] = {}, z[V] = {}, tv[V] = {}, h[V] = {};
            load_unit_once<V>(X + at, x);  // every load of the unit before the first use: one wait
            load_unit_once<V>(PH + at, p);
            if (whole) {
                load_unit_once<V>(R + at, s);
                if (kJac) load_unit_once<V>(SH + at, z);
                load_unit_once<V>(TT + at, tv);
                load_unit_once<V>(RH + at, h);
            }
#pragma unroll
            for (int q = 0; q < V; ++q) {
                if (step[q] != 0) x[q] = fma(alpha[q], p[q], x[q]);
                if (step[q] == 2) {
                    x[q] = fma(omega[q], kJac ? z[q] : s[q], x[q]);
                    s[q] = fma(-omega[q], tv[q], s[q]);
                    rr[q] = s[q] * s[q], hh[q] = h[q] * s[q];
                }
            }
            store_unit_once<V>(X + at, x);
            if (whole) store_unit_once<V>(R + at, s);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = rr[q], hr[i * V + q] = hh[q];
    }
    unit_partials<K>(prod, true, hr, true, partials, count);
}

// The running columns: p = fma(beta, fma(-omega, v, p), r) ; p^ = dinv p
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void bicg_multi_direction_kernel(long long n, const BicgMultiColumn* __restrict__ cols,
                                                                     const double* __restrict__ VV, const double* __restrict__ R,
                                                                     const double* __restrict__ dinv, double* __restrict__ P,
                                                                     double* __restrict__ PH) {
    bool need = false;
#pragma unroll
    for (int j = 0; j < K; ++j) need = need || running(cols[j]);
    if (!need) return;  // uniform over the launch
    BICG_MULTI_UNITS {
        BICG_MULTI_UNIT;
        bool run[V], any = false, all = true;
        double omega[V], beta[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const BicgMultiColumn& c = cols[col0 + q];
            run[q] = running(c), omega[q] = c.omega, beta[q] = c.beta;
            any = any || run[q], all = all && run[q];
        }
        if (!any || !inside) continue;
        double p[V], v[V], r[V], keep[V] = {};
        load_unit_once<V>(P + at, p);
        load_unit_once<V>(VV + at, v);
        load_unit_once<V>(R + at, r);
        const double dv = kJac ? dinv[row0 + t] : 1.0;
        if (kJac && !all) load_row<V>(PH + at, keep);  // a stopped column beside a running one: its bits go back as they came
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (run[q]) p[q] = fma(beta[q], fma(-omega[q], v[q], p[q]), r[q]);
        if (kJac) {
            double h[V];
#pragma unroll
            for (int q = 0; q < V; ++q) h[q] = run[q] ? dv * p[q] : keep[q];
            store_unit_once<V>(P + at, p);
            store_row<V>(PH + at, h);  // plain: the next SpMM reads it
        } else {
            store_row<V>(P + at, p);  // plain: p^ is p, the next SpMM reads it
        }
    }
}
#undef BICG_MULTI_UNITS
#undef BICG_MULTI_UNIT

// ---- the scalar steps: bicgstab.hip's bicg_step, per column and branch for branch. which: 0 = r0.r0, 1 = sigma, 2 = s.s,
// 3 = t.s / t.t, 4 = r.r / r^0.r. `stop` of the single solver is `done` here; step 1 sets `active`, and steps 2 to 4 pass over a
// column that is not running. ----
__device__ __forceinline__ void bicg_multi_record(BicgMultiColumn& c, double norm, double* hist, int hist_cap) {
    c.iterations += 1;
    c.residual = norm;
    if (c.iterations < hist_cap) hist[c.iterations] = norm;
}

__device__ void bicg_multi_step(BicgMultiColumn& c, int which, const double* total, double tol, double* hist, int hist_cap) {
    if (which == 0) {
        c.rho = total[0];
        c.b_norm = sqrt(total[0]);
        c.residual = c.b_norm;
        c.sigma = c.alpha = c.omega = c.beta = c.s_norm = 0.0;
        c.active = c.done = c.iterations = c.converged = c.breakdown = c.x_step = c.pad[0] = c.pad[1] = 0;
        if (hist_cap > 0) hist[0] = c.b_norm;
    } else if (which == 1) {
        c.active = c.done ? 0 : 1;
        if (!c.active) return;  // frozen: the kernels pass over it, x_step and the rest keep their bits
        c.sigma = total[0];
        if (usable(c.sigma)) {
            c.alpha = c.rho / c.sigma;
            c.x_step = 2;
        } else {
            c.alpha = 0.0;
            c.x_step = 0;
            c.breakdown = 1, c.done = 1;
            bicg_multi_record(c, c.residual, hist, hist_cap);
        }
    } else if (!running(c)) {
        return;
    } else if (which == 2) {
        c.s_norm = sqrt(total[0]);
        if (c.s_norm / c.b_norm < tol) {
            c.x_step = 1;
            c.converged = 1, c.done = 1;
            bicg_multi_record(c, c.s_norm, hist, hist_cap);
        }
    } else if (which == 3) {
        if (usable(total[0]) && usable(total[1])) {
            c.omega = total[0] / total[1];
        } else {
            c.omega = 0.0;
            c.x_step = 1;
            c.breakdown = 2, c.done = 1;
            bicg_multi_record(c, c.s_norm, hist, hist_cap);
        }
    } else {
        const double res = sqrt(total[0]);
        bicg_multi_record(c, res, hist, hist_cap);
        if (res / c.b_norm < tol) {
            c.converged = 1, c.done = 1;
        } else if (!usable(total[1])) {
            c.breakdown = 3, c.done = 1;
        } else {
            c.beta = (total[1] / c.rho) * (c.alpha / c.omega);
            c.rho = total[1];
        }
    }
}

// Stage 2 of each value + the scalar step of column j (workgroup j). Value v of column j: slices[(v * k + j) * slice_count ...].
__global__ __launch_bounds__(kBlock) void bicg_multi_step_kernel(const double* __restrict__ slices, int slice_count, int k, int nv, int which,
                                                                double tol, BicgMultiColumn* __restrict__ cols, double* __restrict__ hist,
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
    if (threadIdx.x == 0) bicg_multi_step(cols[j], which, total, tol, hist + (long long)j * hist_cap, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_bicgstab_multi_stage ----

// What the launches of one solve (or one stage call) work on. "none": PH == P and SH == R.
struct VecArgs {
    bool jac;
    long long n;
    const BicgMultiColumn* cols;
    const double* dinv;
    double *X, *R, *RH, *P, *PH, *SH, *V, *T;
    double* partials;
    long long count;  // the workgroups of a launch, (n + 255) / 256
};
enum { kStageInit, kStageDotRv, kStageUpdateS, kStageDotT, kStageUpdateXr, kStageDirection };

template <int K, bool kJac>
void launch_vec_kind(int stage, const VecArgs& a) {
    const dim3 grid((unsigned)a.count), block(kBlock);
    if (stage == kStageInit)
        hipLaunchKernelGGL((bicg_multi_init_kernel<K, kJac>), grid, block, 0, kBatchStream, a.n, a.V, a.dinv, a.R, a.RH, a.P, a.PH, a.partials,
                           a.count);
    else if (stage == kStageUpdateS)
        hipLaunchKernelGGL((bicg_multi_update_s_kernel<K, kJac>), grid, block, 0, kBatchStream, a.n, a.cols, a.V, a.dinv, a.R, a.SH, a.partials,
                           a.count);
    else if (stage == kStageUpdateXr)
        hipLaunchKernelGGL((bicg_multi_update_xr_kernel<K, kJac>), grid, block, 0, kBatchStream, a.n, a.cols, a.PH, a.SH, a.T, a.RH, a.X, a.R,
                           a.partials, a.count);
    else
        hipLaunchKernelGGL((bicg_multi_direction_kernel<K, kJac>), grid, block, 0, kBatchStream, a.n, a.cols, a.V, a.R, a.dinv, a.P, a.PH);
}

template <int K>
void launch_vec(int stage, const VecArgs& a) {
    const dim3 grid((unsigned)a.count), block(kBlock);
    if (stage == kStageDotRv)
        hipLaunchKernelGGL((bicg_multi_dot_rv_kernel<K>), grid, block, 0, kBatchStream, a.n, a.cols, a.RH, a.V, a.partials, a.count);
    else if (stage == kStageDotT)
        hipLaunchKernelGGL((bicg_multi_dot_t_kernel<K>), grid, block, 0, kBatchStream, a.n, a.cols, a.T, a.R, a.partials, a.count);
    else if (a.jac)
        launch_vec_kind<K, true>(stage, a);
    else
        launch_vec_kind<K, false>(stage, a);
}

void launch_vector_stage(int k, int stage, const VecArgs& a) {
    auto launch = [&](auto K) { launch_vec<decltype(K)::value>(stage, a); };
    if (!dispatch_k(k, launch)) launch(std::integral_constant<int, kMaxRhs>{});
}

int values_of_step(int which) { return which >= 3 ? 2 : 1; }

// The two reduction launches behind a scalar step: nv x k x slices_for(count) slice sums of the values at `partials` (value v of
// column j at [(v * k + j) * count ...]), then per column their sums and step `which`. slices: 2 k x slices_for(count) doubles.
void launch_reduce(int k, const double* partials, long long count, double* slices, int which, double tol, BicgMultiColumn* cols, double* hist,
                   int hist_cap) {
    const int sc = slices_for(count), nv = values_of_step(which);
    hipLaunchKernelGGL(multi_reduce_slices_kernel, dim3((unsigned)sc, (unsigned)(nv * k)), dim3(kBlock), 0, kBatchStream, partials, count, sc, slices);
    hipLaunchKernelGGL(bicg_multi_step_kernel, dim3((unsigned)k), dim3(kBlock), 0, kBatchStream, slices, sc, k, nv, which, tol, cols, hist, hist_cap);
}

bool fail(const char* what) { return batched_fail(kTag, what); }

// ---- workspace: the batched scaffold's X, R, P, AP (here V), partials for two values, slices, column records and histories, and
// next to them r^0 and T; "jacobi": P^ and S^ as well. Kept between calls, released with the other CG workspaces. ----
struct BicgMultiWorkspace : BatchedWorkspace<BicgMultiColumn> {
    double *RH = nullptr, *T = nullptr;
    double *PH = nullptr, *SH = nullptr;  // kind "jacobi" only: they join with its first solve

    BicgMultiWorkspace() : BatchedWorkspace<BicgMultiColumn>(2) {}  // two dot-product values per launch: t.s / t.t, r.r / r^0.r

    void release() {
        device_release(RH);
        device_release(T);
        device_release(PH);
        device_release(SH);
        BatchedWorkspace<BicgMultiColumn>::release();
    }

    size_t bytes() const {
        if (X == nullptr) return 0;
        return BatchedWorkspace<BicgMultiColumn>::bytes() + (PH != nullptr ? 4 : 2) * (size_t)n * k * sizeof(double);
    }

    bool ensure(int n_, int k_, int device_, long long partial_cap_, int hist_cap_, bool jac) {
        if (X != nullptr && (n != n_ || k != k_ || device != device_ || partial_cap < partial_cap_)) release();
        if (!BatchedWorkspace<BicgMultiColumn>::ensure(kTag, n_, k_, device_, partial_cap_, hist_cap_, false)) return false;
        const size_t count = (size_t)n_ * k_, vec = count * sizeof(double);
        char what[64];
        snprintf(what, sizeof what, "%d systems of %d rows%s", k_, n_, jac ? " (jacobi)" : "");
        if (RH == nullptr) {
            if (!device_has_room(2 * vec + ((size_t)64 << 20), kTag, what)) return release(), false;
            RH = device_try_alloc<double>(count);
            T = device_try_alloc<double>(count);
            if (!RH || !T) {
                release();
                return fail("the workspace could not be allocated: refused");
            }
        }
        if (jac && PH == nullptr) {
            if (!device_has_room(2 * vec + ((size_t)64 << 20), kTag, what)) return false;
            PH = device_try_alloc<double>(count);
            SH = device_try_alloc<double>(count);
            if (!PH || !SH) {
                device_release(PH);
                device_release(SH);
                return fail("the Jacobi block vectors could not be allocated: refused");
            }
            // S^ is read by the second SpMM of an iteration in which no column reached the s kernel (bicgstab.hip gives the reason)
            HIP_CHECK(hipMemsetAsync(SH, 0, vec, kBatchStream));
        }
        return true;
    }
};
BicgMultiWorkspace g_ws;
std::vector<std::vector<double>> g_history;  // of the last batched BiCGSTAB solve, per column

ColumnSummary summary_of(const BicgMultiColumn& c) {
    static const char* const scalar[] = {nullptr, "sigma = r^.v", "t.t or t.s", "rho' = r^.r"};
    return {c.iterations, c.converged != 0, c.breakdown != 0, c.residual, c.b_norm, c.active != 0, scalar[c.breakdown & 3]};
}

}  // namespace

namespace spmv_amd {
void release_bicgstab_multi_workspace_locked() { g_ws.release(); }
size_t bicgstab_multi_workspace_bytes_locked() { return g_ws.bytes(); }
}  // namespace spmv_amd

extern "C" int spmv_amd_bicgstab_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int nrhs, const double* B,
                                                    double* X, const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (op == nullptr || m == nullptr) return fail("null argument"), 1;  // the two pointers the shared checks do not name so
    if (!check_rhs(kTag, nrhs)) return 1;
    if (m->kind != kNone && m->kind != kJacobi) {
        fprintf(stderr,
                "[%s] preconditioner kind '%s' is built for symmetric definite matrices: BiCGSTAB takes 'none' or 'jacobi': refused\n", kTag,
                spmv_amd_precond_kind(m));
        return 1;
    }
    MultiOperand o;
    if (!check_batched_system(kTag, kTag, op, mat, nrhs, B, X, config, stats, &o)) return 1;
    if (m->n != mat->rows) {
        fprintf(stderr, "[%s] the preconditioner is for %d rows, mat->rows = %d\n", kTag, m->n, mat->rows);
        return 1;
    }
    if (!precond_matches(op, m, diagonal_source_of(op))) return fail("the preconditioner does not belong to this operator as it stands: refused"), 1;
    const int n = mat->rows, k = nrhs;
    const CGConfig cfg = *config;
    const bool jac = m->kind == kJacobi;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const long long vec_count = ((long long)n + kBlock - 1) / kBlock;
    BicgMultiWorkspace& w = g_ws;
    if (!w.ensure(n, k, device, vec_count, cfg.max_iters + 1, jac)) return 1;
    load_block_system(w, k, n, B, X, true);  // the records as zeros: done = 0, so the first iteration's kernels run

    std::vector<ColumnSummary> cols;
    StageTimers T(cfg.enable_detailed_timers != 0, kBatchStream);
    VecArgs a{};
    a.jac = jac, a.n = n, a.cols = w.cols, a.dinv = jac ? m->dinv : nullptr, a.X = w.X, a.R = w.R, a.RH = w.RH, a.P = w.P;
    a.PH = jac ? w.PH : w.P, a.SH = jac ? w.SH : w.R, a.V = w.AP, a.T = w.T, a.partials = w.partials, a.count = vec_count;
    auto vec = [&](int stage) { T.run(&T.t_blas, [&] { launch_vector_stage(k, stage, a); }); };
    auto reduce = [&](int which) {
        T.run(&T.t_red, [&] { launch_reduce(k, w.partials, vec_count, w.slices, which, cfg.tolerance, w.cols, w.hist, w.hist_cap); });
    };
    auto spmm = [&](const double* in, double* out) { T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, in, out, nullptr, kBatchStream); }); };

    T.total.begin(kBatchStream);
    spmm(w.X, a.V);
    vec(kStageInit);
    reduce(0);
    read_columns(w, k, summary_of, cols);
    if (cfg.verbose >= 1) print_initial_residuals(kTag, cols, spmv_amd_precond_kind(m));
    for (int it = 0; it < cfg.max_iters && any_column_running(cols); ++it) {
        spmm(a.PH, a.V);  // V = A P^
        vec(kStageDotRv);
        reduce(1);  // sigma, alpha -- or the first verdict
        vec(kStageUpdateS);
        reduce(2);  // ||s||, the half step's verdict
        spmm(a.SH, a.T);  // T = A S^: for all columns, ignored by the stopped ones
        vec(kStageDotT);
        reduce(3);  // omega
        vec(kStageUpdateXr);
        reduce(4);  // ||r||, the stopping test, rho' and beta
        vec(kStageDirection);
        read_columns(w, k, summary_of, cols);  // synchronises: the one blocking read of the iteration
        if (cfg.verbose >= 2) print_iteration(kTag, cols);
    }
    T.total.end(kBatchStream);
    finish_batched_solve(kTag, w, k, n, X, stats, cfg, T, T.total.elapsed_ms(), cols, g_history);
    return 0;
}

extern "C" size_t spmv_amd_bicgstab_multi_workspace_bytes(void) {
    CgWorkspaceScope scope;
    return bicgstab_multi_workspace_bytes_locked();
}

extern "C" int spmv_amd_bicgstab_last_history_multi(int rhs, double* out, int cap) {
    if (rhs < 0 || rhs >= (int)g_history.size()) return -1;
    return copy_history(g_history[(size_t)rhs], out, cap);
}

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_bicgstab_multi_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdBicgstabMultiColumn) == sizeof(BicgMultiColumn) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, rho) == offsetof(BicgMultiColumn, rho) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, sigma) == offsetof(BicgMultiColumn, sigma) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, alpha) == offsetof(BicgMultiColumn, alpha) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, omega) == offsetof(BicgMultiColumn, omega) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, beta) == offsetof(BicgMultiColumn, beta) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, b_norm) == offsetof(BicgMultiColumn, b_norm) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, residual) == offsetof(BicgMultiColumn, residual) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, s_norm) == offsetof(BicgMultiColumn, s_norm) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, active) == offsetof(BicgMultiColumn, active) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, done) == offsetof(BicgMultiColumn, done) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, iterations) == offsetof(BicgMultiColumn, iterations) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, converged) == offsetof(BicgMultiColumn, converged) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, breakdown) == offsetof(BicgMultiColumn, breakdown) &&
                  offsetof(SpmvAmdBicgstabMultiColumn, x_step) == offsetof(BicgMultiColumn, x_step),
              "lab.h's column record is the device record, field for field");

extern "C" int spmv_amd_bicgstab_multi_stage(const char* stage, const char* kind, int k, SpmvAmdBicgstabMultiStageArgs* a) {
    // argument checks: all before the first HIP call. 16: a block vector the vector kernels access in 16-byte pairs
    static const char* const kStages = "init, dot_rv, update_s, dot_t, update_xr, direction, reduce";
    char names[96];
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    int st;
    if (stage == nullptr) {
        snprintf(names, sizeof names, "no stage named (%s)", kStages);
        return refuse(names), 1;
    }
    if (!strcmp(stage, "init")) st = kStageInit;
    else if (!strcmp(stage, "dot_rv")) st = kStageDotRv;
    else if (!strcmp(stage, "update_s")) st = kStageUpdateS;
    else if (!strcmp(stage, "dot_t")) st = kStageDotT;
    else if (!strcmp(stage, "update_xr")) st = kStageUpdateXr;
    else if (!strcmp(stage, "direction")) st = kStageDirection;
    else if (!strcmp(stage, "reduce")) st = -1;
    else {
        snprintf(names, sizeof names, "unknown stage (%s)", kStages);
        return refuse(names), 1;
    }
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    bool jac = false;
    if (st == -1) {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 4) return refuse("which is not 0 to 4"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (!pointer("partials", a->partials, 8) || !pointer("cols", a->cols, 8)) return 1;
        if (a->hist_cap > 0 && !pointer("hist", a->hist, 8)) return 1;
    } else {
        if (st != kStageDotRv && st != kStageDotT) {
            if (kind == nullptr) return refuse("no preconditioner kind named (none, jacobi)"), 1;
            if (!strcmp(kind, "jacobi")) jac = true;
            else if (strcmp(kind, "none") != 0) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
        }
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
        if (jac && st != kStageUpdateXr && !pointer("dinv", a->dinv, 8)) return 1;
        if (st != kStageInit && !pointer("cols", a->cols, 8)) return 1;
        if (st != kStageDirection && !pointer("partials", a->partials, 8)) return 1;
        if (st != kStageDotRv && !pointer("R", a->R, 16)) return 1;
        if ((st == kStageInit || st == kStageDotRv || st == kStageUpdateXr) && !pointer("RH", a->RH, 16)) return 1;
        if ((st == kStageInit || st == kStageDirection || (st == kStageUpdateXr && !jac)) && !pointer("P", a->P, 16)) return 1;
        if (jac && (st == kStageInit || st == kStageDirection || st == kStageUpdateXr) && !pointer("PH", a->PH, 16)) return 1;
        if (jac && (st == kStageUpdateS || st == kStageUpdateXr) && !pointer("SH", a->SH, 16)) return 1;
        if ((st == kStageInit || st == kStageDotRv || st == kStageUpdateS || st == kStageDirection) && !pointer("V", a->V, 16)) return 1;
        if ((st == kStageDotT || st == kStageUpdateXr) && !pointer("T", a->T, 16)) return 1;
        if (st == kStageUpdateXr && !pointer("X", a->X, 16)) return 1;
    }

    BicgMultiColumn* cols = reinterpret_cast<BicgMultiColumn*>(a->cols);
    double* slices = nullptr;
    if (st == -1) {
        slices = device_alloc<double>(2 * (size_t)k * slices_for(a->count));
        launch_reduce(k, a->partials, a->count, slices, a->which, a->tol, cols, a->hist, a->hist_cap);
    } else {
        VecArgs v{};
        v.jac = jac, v.n = (long long)a->n, v.cols = cols, v.dinv = a->dinv, v.X = a->X, v.R = a->R, v.RH = a->RH, v.P = a->P;
        v.PH = jac ? a->PH : a->P, v.SH = jac ? a->SH : a->R, v.V = a->V, v.T = a->T, v.partials = a->partials;
        v.count = (v.n + kBlock - 1) / kBlock;
        launch_vector_stage(k, st, v);
        a->count = v.count;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    device_release(slices);
    return 0;
}
#endif  // SPMV_AMD_LAB
