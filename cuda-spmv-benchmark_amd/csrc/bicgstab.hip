// bicgstab.hip -- right-preconditioned BiCGSTAB over any SpmvOperator: the solver for matrices that are not symmetric definite
// (DESIGN.md section 21). It asks run_device of the operator and nothing else; kinds "none" and "jacobi" (precond.hip's preconditioner
// record; "chebyshev" and "multigrid" are built for symmetric definite matrices and refused). Contract, statistics, timer rule,
// verbose semantics and stopping rule are spmv_amd_pcg_solve_device's (solve_common.hpp); right preconditioning keeps the recorded
// residual the true one.
//
// The algebra (dinv is Jacobi's, a hat means "times dinv" -- kind "none": the same vector, kept in ONE buffer; every fma is explicit,
// every other operation rounds once, the file is compiled with -ffp-contract=off):
//   r = fma(1.0, b, -1.0 * (A x0)) ; r^ = r ; p = r ; p^ = dinv p ; rho = r.r ; ||r0|| = sqrt(rho) ; history[0] = ||r0||
//   1. v = A p^                                                      (the operator's own bits)
//   2. sigma = r^.v ; zero or not finite: BREAKDOWN -- the iteration is counted, the unchanged residual recorded, nothing updated
//   3. alpha = rho / sigma ; s = fma(-alpha, v, r) ; s^ = dinv s ; ||s|| = sqrt(s.s)
//   4. ||s|| / ||r0|| < tol: HALF STEP -- x = fma(alpha, p^, x), the iteration counted, ||s|| recorded, converged
//   5. t = A s^ ; omega = (t.s) / (t.t) ; t.t or t.s zero or not finite: BREAKDOWN -- x = fma(alpha, p^, x), r = s, ||s|| recorded,
//      the iteration counted
//   6. x = fma(omega, s^, fma(alpha, p^, x)) ; r = fma(-omega, t, s) ; ||r|| = sqrt(r.r) recorded, the iteration counted, then the
//      strict stopping test
//   7. rho' = r^.r ; zero or not finite: BREAKDOWN, x and r keep their update ; else beta = (rho' / rho) * (alpha / omega) ;
//      rho = rho' ; p = fma(beta, fma(-omega, v, p), r) ; p^ = dinv p
// A breakdown ends the solve with converged = 0; there is no sign test.
//
// Launches per iteration (streaming kernels in pcg.hip's style: one-wave workgroups on stream_grid(n), one 16-byte pair per lane, the
// odd last element by lane 0 of workgroup 0 after its pair, the loads before the scalars, wave_sum, two values side by side at
// partials[g] and partials[count + g]); each sum and its scalar step are ONE launch of bicg_reduce_kernel, pcg_reduce_kernel's
// geometry on reduce_device.hpp's helpers:
//   the product v = A p^ | partials of r^.v (16 B/row) + sum | the s kernel: r -= alpha v in place (r now holds s), s.s partials,
//   "jacobi": s^ written + sum | the product t = A s^ | partials of t.s and t.t (16) + sum | the x / r kernel: step 6 with the
//   partials of r.r and r^.r + sum | the direction kernel: step 7
// then ONE small blocking read of the scalar record. Every kernel behind a verdict tests the record's `stop` (the x / r kernel its
// `x_step`) and returns at once, so the second product of a half-step or breakdown iteration runs and is ignored: one wasted SpMV
// in the last iteration only, and no second blocking read. Bytes per interior row and iteration on stencil5-csr:
// 2 x 56 + 16 + 24 + 16 + 56 + 32 = 256 ("none"); "jacobi" 296: the s kernel and the direction kernel read dinv and write s^ / p^
// (16 each), the x / r kernel reads s^ beside s (8). Workspace: x, b, r, r^, p, v, t; "jacobi": p^ and s^ as well.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "precond.hpp"
#include "reduce_device.hpp"
#include "single_solve.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

// Device scalars of one solve.
struct BicgScalars {
    double rho;       // r^.r of the current residual
    double sigma, alpha, omega, beta;
    double b_norm;    // ||r0||
    double residual;  // the norm recorded last
    double s_norm;    // ||s|| of this iteration
    int iterations;
    int converged;    // stopping test met (by the half step or by the whole one)
    int breakdown;    // 0, or which scalar stopped the solve: 1 sigma, 2 omega (t.t or t.s), 3 rho'
    int x_step;       // what the x / r kernel applies in this iteration: 0 nothing, 1 the half step, 2 the whole step
    int stop;         // the verdict: set with converged or breakdown; kernels behind it return at once
    int pad;
};

// ---- the streaming kernels. dinv, phat and shat are not looked at by the "none" instantiations (p^ is p, s^ is r). ----

// r = fma(1.0, b, -1.0 * Ax) ; r^ = r ; p = r ; p^ = dinv p ; partials of r.r
template <bool kJac>
__global__ __launch_bounds__(kWave) void bicg_init_kernel(size_t n, const double* __restrict__ b, const double* __restrict__ Ax,
                                                          const double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ rhat,
                                                          double* __restrict__ p, double* __restrict__ phat, double* __restrict__ partials) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    double rr = 0.0;
    if (i < (n >> 1)) {
        const d2 bv = load_once(b, i), av = load_once(Ax, i);
        d2 rv;
        rv.x = fma(1.0, bv.x, -1.0 * av.x);
        rv.y = fma(1.0, bv.y, -1.0 * av.y);
        store_once(r, i, rv);
        store_once(rhat, i, rv);
        if (kJac) {
            const d2 dv = load_once(dinv, i);
            d2 hv;
            hv.x = dv.x * rv.x, hv.y = dv.y * rv.y;
            store_once(p, i, rv);
            reinterpret_cast<d2*>(phat)[i] = hv;  // plain: the first product reads it
        } else {
            reinterpret_cast<d2*>(p)[i] = rv;
        }
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rl = fma(1.0, b[n - 1], -1.0 * Ax[n - 1]);
        r[n - 1] = rl, rhat[n - 1] = rl, p[n - 1] = rl;
        if (kJac) phat[n - 1] = dinv[n - 1] * rl;
        rr = fma(rl, rl, rr);
    }
    rr = wave_sum(rr);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr;
}

// The partials of a.b (value 0) and, kTwo, of a.a (value 1). kTwo (t.s and t.t) lies behind a verdict; the r^.v pass does not.
template <bool kTwo>
__global__ __launch_bounds__(kWave) void bicg_dot_kernel(size_t n, const BicgScalars* __restrict__ s, const double* __restrict__ a,
                                                         const double* __restrict__ b, double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 av = {0.0, 0.0}, bv = {0.0, 0.0};
    if (live) av = load_once(a, i), bv = load_once(b, i);  // the loads before the scalars
    if (kTwo && s->stop != 0) return;
    double ab = 0.0, aa = 0.0;
    if (live) {
        ab = fma(av.x, bv.x, ab), ab = fma(av.y, bv.y, ab);
        if (kTwo) aa = fma(av.x, av.x, aa), aa = fma(av.y, av.y, aa);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double al = a[n - 1];
        ab = fma(al, b[n - 1], ab);
        if (kTwo) aa = fma(al, al, aa);
    }
    ab = wave_sum(ab);
    if (kTwo) aa = wave_sum(aa);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = ab;
        if (kTwo) partials[count + blockIdx.x] = aa;
    }
}

// s = fma(-alpha, v, r) in place (r holds s from here to the x / r kernel) ; s^ = dinv s ; partials of s.s
template <bool kJac>
__global__ __launch_bounds__(kWave) void bicg_update_s_kernel(size_t n, const BicgScalars* __restrict__ s, const double* __restrict__ v,
                                                              const double* __restrict__ dinv, double* __restrict__ r,
                                                              double* __restrict__ shat, double* __restrict__ partials) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 vv = {0.0, 0.0}, rv = {0.0, 0.0}, dv = {1.0, 1.0};
    if (live) {  // the loads before the scalars
        vv = load_once(v, i);
        rv = load_once(r, i);
        if (kJac) dv = load_once(dinv, i);
    }
    if (s->stop != 0) return;
    const double alpha = s->alpha;
    double ss = 0.0;
    if (live) {
        rv.x = fma(-alpha, vv.x, rv.x);
        rv.y = fma(-alpha, vv.y, rv.y);
        if (kJac) {
            d2 hv;
            hv.x = dv.x * rv.x, hv.y = dv.y * rv.y;
            store_once(r, i, rv);
            reinterpret_cast<d2*>(shat)[i] = hv;  // plain: the second product reads it
        } else {
            reinterpret_cast<d2*>(r)[i] = rv;
        }
        ss = fma(rv.x, rv.x, ss), ss = fma(rv.y, rv.y, ss);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double sl = fma(-alpha, v[n - 1], r[n - 1]);
        r[n - 1] = sl;
        if (kJac) shat[n - 1] = dinv[n - 1] * sl;
        ss = fma(sl, sl, ss);
    }
    ss = wave_sum(ss);
    if (threadIdx.x == 0) partials[blockIdx.x] = ss;
}

// x_step 2: x = fma(omega, s^, fma(alpha, p^, x)) ; r = fma(-omega, t, s) in place ; partials of r.r and r^.r.
// x_step 1 (half step, omega breakdown): x = fma(alpha, p^, x) alone, r keeps s. x_step 0 (sigma breakdown): nothing.
template <bool kJac>
__global__ __launch_bounds__(kWave) void bicg_update_xr_kernel(size_t n, const BicgScalars* __restrict__ s, const double* __restrict__ phat,
                                                               const double* __restrict__ shat, const double* __restrict__ t,
                                                               const double* __restrict__ rhat, double* __restrict__ x,
                                                               double* __restrict__ r, double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 xv = {0.0, 0.0}, pv = {0.0, 0.0}, sv = {0.0, 0.0}, zv = {0.0, 0.0}, tv = {0.0, 0.0}, hv = {0.0, 0.0};
    if (live) {  // the loads before the scalars
        xv = load_once(x, i);
        pv = load_once(phat, i);
        sv = load_once(r, i);
        if (kJac) zv = load_once(shat, i);
        tv = load_once(t, i);
        hv = load_once(rhat, i);
    }
    const int step = s->x_step;
    if (step == 0) return;
    const double alpha = s->alpha, omega = s->omega;
    double rr = 0.0, hr = 0.0;
    if (live) {
        if (!kJac) zv = sv;
        xv.x = fma(alpha, pv.x, xv.x);
        xv.y = fma(alpha, pv.y, xv.y);
        if (step == 2) {
            xv.x = fma(omega, zv.x, xv.x);
            xv.y = fma(omega, zv.y, xv.y);
            sv.x = fma(-omega, tv.x, sv.x);
            sv.y = fma(-omega, tv.y, sv.y);
            store_once(r, i, sv);
            rr = fma(sv.x, sv.x, rr), rr = fma(sv.y, sv.y, rr);
            hr = fma(hv.x, sv.x, hr), hr = fma(hv.y, sv.y, hr);
        }
        store_once(x, i, xv);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double xl = fma(alpha, phat[n - 1], x[n - 1]);
        if (step == 2) {
            const double sl = r[n - 1];
            xl = fma(omega, kJac ? shat[n - 1] : sl, xl);
            const double rl = fma(-omega, t[n - 1], sl);
            r[n - 1] = rl;
            rr = fma(rl, rl, rr), hr = fma(rhat[n - 1], rl, hr);
        }
        x[n - 1] = xl;
    }
    if (step != 2) return;
    rr = wave_sum(rr), hr = wave_sum(hr);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr, partials[count + blockIdx.x] = hr;
}

// p = fma(beta, fma(-omega, v, p), r) ; p^ = dinv p
template <bool kJac>
__global__ __launch_bounds__(kWave) void bicg_direction_kernel(size_t n, const BicgScalars* __restrict__ s, const double* __restrict__ v,
                                                               const double* __restrict__ r, const double* __restrict__ dinv,
                                                               double* __restrict__ p, double* __restrict__ phat) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 pv = {0.0, 0.0}, vv = {0.0, 0.0}, rv = {0.0, 0.0}, dv = {1.0, 1.0};
    if (live) {  // the loads before the scalars
        pv = load_once(p, i);
        vv = load_once(v, i);
        rv = load_once(r, i);
        if (kJac) dv = load_once(dinv, i);
    }
    if (s->stop != 0) return;
    const double omega = s->omega, beta = s->beta;
    if (live) {
        pv.x = fma(beta, fma(-omega, vv.x, pv.x), rv.x);
        pv.y = fma(beta, fma(-omega, vv.y, pv.y), rv.y);
        if (kJac) {
            d2 hv;
            hv.x = dv.x * pv.x, hv.y = dv.y * pv.y;
            store_once(p, i, pv);
            reinterpret_cast<d2*>(phat)[i] = hv;  // plain: the next product reads it
        } else {
            reinterpret_cast<d2*>(p)[i] = pv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double pl = fma(beta, fma(-omega, v[n - 1], p[n - 1]), r[n - 1]);
        p[n - 1] = pl;
        if (kJac) phat[n - 1] = dinv[n - 1] * pl;
    }
}

// ---- reductions: NV (1 or 2) sums of `count` partials each (value v at partials[v * count ...]) in ONE launch, then the scalar
// step. pcg_reduce_kernel's geometry: one workgroup up to 1024 partials, else slice workgroups that publish their slice sums of
// value 0 into the stage's `sums`, of value 1 into its `extra` slots, and the workgroup that draws the last ticket sums both and
// takes the step. which: 0 = r0.r0, 1 = sigma, 2 = s.s, 3 = t.s / t.t, 4 = r.r / r^.r. Steps 2 to 4 lie behind a verdict: every
// workgroup reads `stop` before it draws a ticket, and the step writes it only after the last ticket is drawn. ----

__device__ __forceinline__ void bicg_record(BicgScalars* s, double norm, double* hist, int hist_cap) {
    s->iterations += 1;
    s->residual = norm;
    if (s->iterations < hist_cap) hist[s->iterations] = norm;
}

__device__ void bicg_step(BicgScalars* s, int which, const double* total, double tol, double* hist, int hist_cap) {
    if (which == 0) {
        s->rho = total[0];
        s->b_norm = sqrt(total[0]);
        s->residual = s->b_norm;
        s->sigma = s->alpha = s->omega = s->beta = s->s_norm = 0.0;
        s->iterations = s->converged = s->breakdown = s->x_step = s->stop = s->pad = 0;
        if (hist_cap > 0) hist[0] = s->b_norm;
    } else if (which == 1) {
        s->sigma = total[0];
        if (usable(s->sigma)) {
            s->alpha = s->rho / s->sigma;
            s->x_step = 2;
        } else {
            s->alpha = 0.0;
            s->x_step = 0;
            s->breakdown = 1, s->stop = 1;
            bicg_record(s, s->residual, hist, hist_cap);
        }
    } else if (which == 2) {
        s->s_norm = sqrt(total[0]);
        if (s->s_norm / s->b_norm < tol) {
            s->x_step = 1;
            s->converged = 1, s->stop = 1;
            bicg_record(s, s->s_norm, hist, hist_cap);
        }
    } else if (which == 3) {
        if (usable(total[0]) && usable(total[1])) {
            s->omega = total[0] / total[1];
        } else {
            s->omega = 0.0;
            s->x_step = 1;
            s->breakdown = 2, s->stop = 1;
            bicg_record(s, s->s_norm, hist, hist_cap);
        }
    } else {
        const double res = sqrt(total[0]);
        bicg_record(s, res, hist, hist_cap);
        if (res / s->b_norm < tol) {
            s->converged = 1, s->stop = 1;
        } else if (!usable(total[1])) {
            s->breakdown = 3, s->stop = 1;
        } else {
            s->beta = (total[1] / s->rho) * (s->alpha / s->omega);
            s->rho = total[1];
        }
    }
}

template <int NV>
__global__ __launch_bounds__(kReduceBlock) void bicg_reduce_kernel(const double* __restrict__ partials, int count, int slice, int blocks,
                                                                   double* stage_base, BicgScalars* s, int which, double tol, double* hist,
                                                                   int hist_cap) {
    __shared__ double sh[kReduceBlock];
    __shared__ int s_last;
    if (which >= 2 && s->stop != 0) return;
    double total[2] = {0.0, 0.0};
    const ReduceStage stage = reduce_stage_of(stage_base);
    const auto slot_of = [&](int v) { return v == 0 ? stage.sums : stage.extra; };
    if (!sum_values_last_block<NV>(partials, count, NV, slice, blocks, stage.ticket, slot_of, sh, &s_last, total)) return;
    if (threadIdx.x == 0) bicg_step(s, which, total, tol, hist, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_bicgstab_stage ----

// What the launches of one solve (or one stage call) work on. "none": phat == p and shat == r.
struct BicgVectors {
    bool jac = false;
    size_t n = 0;
    const double* b = nullptr;
    const double* dinv = nullptr;
    double *x = nullptr, *r = nullptr, *rhat = nullptr, *p = nullptr, *phat = nullptr, *shat = nullptr, *v = nullptr;
    const double* t = nullptr;
    double* partials = nullptr;
    BicgScalars* s = nullptr;
};

#define BICG_LAUNCH(kernel, ...) SPMV_AMD_STREAM_LAUNCH(kernel, a.jac, a.n, __VA_ARGS__)
void launch_bicg_init(const BicgVectors& a) { BICG_LAUNCH(bicg_init_kernel, a.b, a.v, a.dinv, a.r, a.rhat, a.p, a.phat, a.partials); }
void launch_bicg_update_s(const BicgVectors& a) { BICG_LAUNCH(bicg_update_s_kernel, a.s, a.v, a.dinv, a.r, a.shat, a.partials); }
void launch_bicg_update_xr(const BicgVectors& a) {
    BICG_LAUNCH(bicg_update_xr_kernel, a.s, a.phat, a.shat, a.t, a.rhat, a.x, a.r, a.partials, count);
}
void launch_bicg_direction(const BicgVectors& a) { BICG_LAUNCH(bicg_direction_kernel, a.s, a.v, a.r, a.dinv, a.p, a.phat); }
#undef BICG_LAUNCH

void launch_bicg_dot_rv(const BicgVectors& a) {
    const dim3 grid(stream_grid(a.n)), block(kWave);
    hipLaunchKernelGGL(bicg_dot_kernel<false>, grid, block, 0, kStream, a.n, a.s, a.rhat, a.v, a.partials, (int)grid.x);
}
void launch_bicg_dot_t(const BicgVectors& a) {
    const dim3 grid(stream_grid(a.n)), block(kWave);
    hipLaunchKernelGGL(bicg_dot_kernel<true>, grid, block, 0, kStream, a.n, a.s, a.t, a.r, a.partials, (int)grid.x);
}

// the sums of `count` partials per value and the scalar step `which` (0, 1, 2: one value; 3, 4: two)
void launch_bicg_reduce(const double* partials, int count, int which, double* stage, BicgScalars* s, double tol, double* hist, int hist_cap) {
    int slice = 0, blocks = 0;
    reduce_geometry(count, &slice, &blocks);
    if (which < 3)
        hipLaunchKernelGGL(bicg_reduce_kernel<1>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
    else
        hipLaunchKernelGGL(bicg_reduce_kernel<2>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
}

// ---- workspace: kept between calls, released with the other CG workspaces ----
struct BicgWorkspace {
    int n = 0, device = -1;
    double *x = nullptr, *b = nullptr, *r = nullptr, *rhat = nullptr, *p = nullptr, *v = nullptr, *t = nullptr;
    double *phat = nullptr, *shat = nullptr;  // kind "jacobi" only
    double* partials = nullptr;               // 2 x streaming workgroups
    double* stage = nullptr;                  // reduce_scratch_alloc()
    BicgScalars* s = nullptr;
    double* hist = nullptr;
    int hist_cap = 0;
    void release() {
        device_release(phat);
        device_release(shat);
        device_release(x);
        device_release(b);
        device_release(r);
        device_release(rhat);
        device_release(p);
        device_release(v);
        device_release(t);
        device_release(partials);
        device_release(stage);
        device_release(s);
        device_release(hist);
        n = 0, device = -1, hist_cap = 0;
    }
};
BicgWorkspace g_bicg;
std::vector<double> g_bicg_history;  // of the last solve

bool fail(const char* what) {
    fprintf(stderr, "[BICGSTAB] %s\n", what);
    return false;
}

bool ensure_workspace(int n, int device, bool jac, int hist_cap) {
    BicgWorkspace& w = g_bicg;
    if (w.x != nullptr && (w.n != n || w.device != device)) w.release();
    const size_t slots = 2 * (size_t)stream_grid((size_t)n);
    if (w.x == nullptr) {
        const size_t need = 7 * (size_t)n * sizeof(double) + slots * sizeof(double) + (size_t)hist_cap * sizeof(double) + ((size_t)64 << 20);
        char what[32];
        snprintf(what, sizeof what, "%d rows", n);
        if (!device_has_room(need, "BICGSTAB", what)) return false;
        w.x = device_try_alloc<double>((size_t)n);
        w.b = device_try_alloc<double>((size_t)n);
        w.r = device_try_alloc<double>((size_t)n);
        w.rhat = device_try_alloc<double>((size_t)n);
        w.p = device_try_alloc<double>((size_t)n);
        w.v = device_try_alloc<double>((size_t)n);
        w.t = device_try_alloc<double>((size_t)n);
        w.partials = device_try_alloc<double>(slots);
        w.s = device_try_alloc<BicgScalars>(1);
        if (!w.x || !w.b || !w.r || !w.rhat || !w.p || !w.v || !w.t || !w.partials || !w.s) {
            w.release();
            return fail("the workspace could not be allocated: refused");
        }
        w.stage = reduce_scratch_alloc();
        w.n = n, w.device = device;
    }
    if (jac && w.phat == nullptr) {  // p^ and s^, next to the rest and sized against free memory like it
        char what[48];
        snprintf(what, sizeof what, "%d rows (jacobi)", n);
        if (!device_has_room(2 * (size_t)n * sizeof(double) + ((size_t)64 << 20), "BICGSTAB", what)) return false;
        w.phat = device_try_alloc<double>((size_t)n);
        w.shat = device_try_alloc<double>((size_t)n);
        if (!w.phat || !w.shat) {
            device_release(w.phat);
            device_release(w.shat);
            return fail("the Jacobi vectors could not be allocated: refused");
        }
        // s^ is read by the second product of an iteration whose verdict came before the s kernel wrote it
        HIP_CHECK(hipMemsetAsync(w.shat, 0, (size_t)n * sizeof(double), kStream));
    }
    if (!grow_history(w.hist, w.hist_cap, hist_cap)) return fail("the history could not be allocated: refused");
    return true;
}

}  // namespace

namespace spmv_amd {
void release_bicgstab_workspace_locked() { g_bicg.release(); }
}  // namespace spmv_amd

extern "C" int spmv_amd_bicgstab_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, const double* b, double* x,
                                              const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (!check_solve_arguments("BICGSTAB", op, mat, m, b, x, config, stats)) return 1;
    if (m->kind != kNone && m->kind != kJacobi) {
        fprintf(stderr,
                "[BICGSTAB] preconditioner kind '%s' is built for symmetric definite matrices: BiCGSTAB takes 'none' or 'jacobi': refused\n",
                spmv_amd_precond_kind(m));
        return 1;
    }
    if (!check_solve_system("BICGSTAB", op, mat, m)) return 1;
    const int n = mat->rows;
    const CGConfig cfg = *config;
    const bool jac = m->kind == kJacobi;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    if (!ensure_workspace(n, device, jac, cfg.max_iters + 1)) return 1;
    BicgWorkspace& w = g_bicg;
    upload(w.b, b, (size_t)n);
    upload(w.x, x, (size_t)n);

    BicgVectors a;
    a.jac = jac, a.n = (size_t)n, a.b = w.b, a.dinv = jac ? m->dinv : nullptr, a.x = w.x, a.r = w.r, a.rhat = w.rhat, a.p = w.p;
    a.phat = jac ? w.phat : w.p, a.shat = jac ? w.shat : w.r, a.v = w.v, a.t = w.t, a.partials = w.partials, a.s = w.s;
    const int count = (int)stream_grid((size_t)n);
    StageTimers T(cfg.enable_detailed_timers != 0, kStream);
    bool failed = false;
    auto product = [&](const double* in, double* out) { timed_product("BICGSTAB", op, T, in, out, failed); };
    auto reduce = [&](int which) {
        T.run(&T.t_red, [&] { launch_bicg_reduce(w.partials, count, which, w.stage, w.s, cfg.tolerance, w.hist, w.hist_cap); });
    };
    BicgScalars h{};

    T.total.begin(kStream);
    product(w.x, w.v);
    if (!failed) {
        T.run(&T.t_blas, [&] { launch_bicg_init(a); });
        reduce(0);
        download(&h, w.s, 1);
        if (cfg.verbose >= 1)
            printf("[BICGSTAB-DEVICE] Initial residual: %e (preconditioner %s)\n", h.b_norm, spmv_amd_precond_kind(m));
    }
    for (int it = 0; it < cfg.max_iters && !failed && !h.converged && !h.breakdown; ++it) {
        product(a.phat, w.v);  // v = A p^
        if (failed) break;
        T.run(&T.t_blas, [&] { launch_bicg_dot_rv(a); });
        reduce(1);  // sigma, alpha -- or the first verdict
        T.run(&T.t_blas, [&] { launch_bicg_update_s(a); });
        reduce(2);  // ||s||, the half step's verdict
        product(a.shat, w.t);  // t = A s^: runs and is ignored behind a verdict
        if (failed) break;
        T.run(&T.t_blas, [&] { launch_bicg_dot_t(a); });
        reduce(3);  // omega
        T.run(&T.t_blas, [&] { launch_bicg_update_xr(a); });
        reduce(4);  // ||r||, the stopping test, rho' and beta
        T.run(&T.t_blas, [&] { launch_bicg_direction(a); });
        download(&h, w.s, 1);  // synchronises: the one blocking read of the iteration
        if (cfg.verbose >= 2)
            printf("[BICGSTAB-DEVICE] Iter %3d: residual = %e (rel = %e)\n", h.iterations, h.residual, h.residual / h.b_norm);
    }
    T.total.end(kStream);
    const double total_ms = T.total.elapsed_ms();
    HIP_CHECK(hipGetLastError());
    if (failed) {
        HIP_CHECK(hipDeviceSynchronize());
        return 1;
    }
    download_solution(x, w.x, n, h.iterations, w.hist, w.hist_cap, g_bicg_history);

    static const char* const scalar[] = {"", "sigma = r^.v", "t.t or t.s", "rho' = r^.r"};
    const SolveSummary done{h.iterations, h.converged != 0, h.residual, h.b_norm, h.breakdown ? scalar[h.breakdown & 3] : nullptr};
    report_solve("BICGSTAB", done, x, n, cfg, T, total_ms, stats);
    return 0;
}

extern "C" int spmv_amd_bicgstab_last_history(double* out, int cap) { return copy_history(g_bicg_history, out, cap); }

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_bicgstab_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdBicgstabScalars) == sizeof(BicgScalars) && offsetof(SpmvAmdBicgstabScalars, b_norm) == offsetof(BicgScalars, b_norm) &&
                  offsetof(SpmvAmdBicgstabScalars, s_norm) == offsetof(BicgScalars, s_norm) &&
                  offsetof(SpmvAmdBicgstabScalars, iterations) == offsetof(BicgScalars, iterations) &&
                  offsetof(SpmvAmdBicgstabScalars, x_step) == offsetof(BicgScalars, x_step) &&
                  offsetof(SpmvAmdBicgstabScalars, stop) == offsetof(BicgScalars, stop),
              "lab.h's scalar record is the device record, field for field");

extern "C" int spmv_amd_bicgstab_stage(const char* stage, const char* kind, SpmvAmdBicgstabStageArgs* a, SpmvAmdBicgstabScalars* scalars) {
    // argument checks: all before the first HIP call. 16: a vector the streaming kernels read or write in 16-byte pairs; 8: an array
    // of doubles read or written one at a time
    static const char* const kStages = "init, dot_rv, update_s, dot_t, update_xr, direction, reduce";
    char names[96];
    auto refuse = [&](const char* what) { return stage_fail("BICGSTAB", stage, what); };
    auto pointer = [&](const char* name, const void* ptr) { return stage_pointer("BICGSTAB", stage, name, ptr, 16); };
    enum { kInit, kDotRv, kUpdateS, kDotT, kUpdateXr, kDirection, kReduce } st;
    if (stage == nullptr) {
        snprintf(names, sizeof names, "no stage named (%s)", kStages);
        return refuse(names), 1;
    }
    if (!strcmp(stage, "init")) st = kInit;
    else if (!strcmp(stage, "dot_rv")) st = kDotRv;
    else if (!strcmp(stage, "update_s")) st = kUpdateS;
    else if (!strcmp(stage, "dot_t")) st = kDotT;
    else if (!strcmp(stage, "update_xr")) st = kUpdateXr;
    else if (!strcmp(stage, "direction")) st = kDirection;
    else if (!strcmp(stage, "reduce")) st = kReduce;
    else {
        snprintf(names, sizeof names, "unknown stage (%s)", kStages);
        return refuse(names), 1;
    }
    if (a == nullptr) return refuse("null arguments"), 1;
    bool jac = false;
    if (st != kReduce) {
        if (st != kDotRv && st != kDotT) {
            const int k = kind_of(kind);
            if (k != kNone && k != kJacobi) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
            jac = k == kJacobi;
        }
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
    }
    if (st != kInit && st != kDotRv && scalars == nullptr) return refuse("null scalar record"), 1;
    const bool needs_dinv = jac && (st == kInit || st == kUpdateS || st == kDirection);
    if (needs_dinv && !pointer("dinv", a->dinv)) return 1;
    if (st == kInit) {
        if (!pointer("b", a->b) || !pointer("v", a->v) || !pointer("r", a->r) || !pointer("rhat", a->rhat) || !pointer("p", a->p) ||
            (jac && !pointer("phat", a->phat)))
            return 1;
    } else if (st == kDotRv) {
        if (!pointer("rhat", a->rhat) || !pointer("v", a->v)) return 1;
    } else if (st == kUpdateS) {
        if (!pointer("v", a->v) || !pointer("r", a->r) || (jac && !pointer("shat", a->shat))) return 1;
    } else if (st == kDotT) {
        if (!pointer("t", a->t) || !pointer("r", a->r)) return 1;
    } else if (st == kUpdateXr) {
        if (!pointer("x", a->x) || !pointer("r", a->r) || !pointer("t", a->t) || !pointer("rhat", a->rhat) ||
            !pointer(jac ? "phat" : "p", jac ? a->phat : a->p) || (jac && !pointer("shat", a->shat)))
            return 1;
    } else if (st == kDirection) {
        if (!pointer("p", a->p) || !pointer("v", a->v) || !pointer("r", a->r) || (jac && !pointer("phat", a->phat))) return 1;
    } else {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 4) return refuse("which is not 0, 1, 2, 3 or 4"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (a->hist_cap > 0 && !stage_pointer("BICGSTAB", stage, "hist", a->hist, 8)) return 1;
    }
    if (st != kDirection && !stage_pointer("BICGSTAB", stage, "partials", a->partials, 8)) return 1;

    BicgScalars h{};
    if (scalars != nullptr) memcpy(&h, scalars, sizeof h);
    BicgScalars* d_s = device_alloc<BicgScalars>(1);
    upload(d_s, &h, 1);
    BicgVectors w;
    w.jac = jac, w.n = a->n, w.b = a->b, w.dinv = a->dinv, w.x = a->x, w.r = a->r, w.rhat = a->rhat, w.p = a->p;
    w.phat = jac ? a->phat : a->p, w.shat = jac ? a->shat : a->r, w.v = a->v, w.t = a->t, w.partials = a->partials, w.s = d_s;
    double* stage_buf = nullptr;
    if (st == kInit) launch_bicg_init(w);
    else if (st == kDotRv) launch_bicg_dot_rv(w);
    else if (st == kUpdateS) launch_bicg_update_s(w);
    else if (st == kDotT) launch_bicg_dot_t(w);
    else if (st == kUpdateXr) launch_bicg_update_xr(w);
    else if (st == kDirection) launch_bicg_direction(w);
    else {
        stage_buf = reduce_scratch_alloc();
        launch_bicg_reduce(a->partials, a->count, a->which, stage_buf, d_s, a->tol, a->hist, a->hist_cap);
    }
    if (st != kReduce) a->count = (int)stream_grid(a->n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (st == kReduce) {
        download(&h, d_s, 1);
        memcpy(scalars, &h, sizeof h);
    }
    device_release(stage_buf);
    device_release(d_s);
    return 0;
}
#endif  // SPMV_AMD_LAB
