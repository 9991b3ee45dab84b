// pcg.hip -- preconditioned CG over any SpmvOperator: kinds "none" and "jacobi" (DESIGN.md section 13), a Chebyshev polynomial in
// D^-1 A (section 14) and one multigrid V-cycle (multigrid.hip, section 15: stencil5-csr; section 17: stencil7-csr).
//
// One loop, spmv_amd_pcg_solve_device: the algebra of cg_solve_device with z = M^-1 r, the same stopping rule (true residual
// ||r_k|| / ||r_0|| < tol, strict, the converging iteration counted), statistics and timer rule (solve_common.hpp has those,
// stream_device.hpp the kernels' small helpers). The loop names every stage all kinds share once:
//   Ap = A p with the p.Ap partials (the operator's fused launch; else run_device + a dot pass) |
//   sum + step (alpha = rz / pAp) |
//   the kind's unit: r -= alpha Ap, ||r|| with history and verdict, z = M^-1 r, beta = rz' / rz; it returns where z is |
//   x += alpha p, p = z + beta p
// then one small blocking read of the scalars (the stopping test; microseconds against milliseconds of work). A kind is a PcgKind:
// two plain functions on the solve's PcgLoop -- `first` (everything before the loop: r0, ||r0||, z0, r0.z0, p0) and `next` (the
// unit above) -- chosen once by pcg_kind_of. No direction ring, no deferred x update, no run-ahead (that is the slab loop's,
// cg_slab.hip). Breakdown: a pAp or r.z' that is zero or not finite stops the loop in that iteration with converged = 0 (no sign
// test: negative-definite systems solve). Sums have a fixed shape (reduce_device.hpp): a solve is bit-reproducible.
//
// "none" / "jacobi" (plain_first, plain_next): z = dinv r (or r) never leaves the registers:
//   r -= alpha Ap with the partials of r.r and r.z | both sums + step (history, verdict, beta) | the x / p kernel applies dinv to r
// Bytes per interior row and iteration on stencil5-csr: 56 (SpMV) + 32 + 48 = 136 ("jacobi"), 120 ("none").
//
// "chebyshev" (cheb_first, cheb_next; degree k, interval [lmin, lmax] of D^-1 A; coefficients c0, h_1, g_1, ... from the host
// recurrence below):
//   term 0:  u = dinv r ; d = c0 u ; z = d
//   step j:  w = A z ; t = fma(-1, w, r) ; u = dinv t ; d = fma(g_j, u, h_j d) ; z = z + d
//   r -= alpha Ap with term 0 in registers, partials of r.r | sum of r.r + verdict, which also lands in a device flag |
//   k steps, each testing that flag before it works: the converging iteration streams nothing | sum of r.z + beta
// A step is cheb_step (declared in precond.hpp), the only place that chooses its form from a ChebSpmv: on a row-lds stencil plan ONE
// launch (spmv_kernels.hip, kMode 3: A z never leaves the registers, z' goes to a second vector; 144 + 88 k bytes per interior row and
// iteration), on any other stencil plan -- 2-D, or a 3-D multigrid level's Stencil7Plan -- the SpMV behind the flag +
// cheb_step_kernel, else run_device + cheb_step_kernel (112 per step). The loop calls it timed, with the flag and the step counter; spmv_amd_precond_apply_device untimed without a flag; the
// multigrid cycle on each of its levels.
//
// "multigrid" (mg_first, mg_next): z = M^-1 r is one V-cycle on the preconditioner's own levels:
//   r -= alpha Ap with the r.r partials (the "none" r update) | sum of r.r + verdict | the host reads the verdict: the converging
//   iteration runs no cycle | V-cycle | sum of r.z + beta
//
// Also here: the set-up passes (diagonal, Gershgorin bound), the creators with their one operator check (creation_source) and the one
// sentence about a bad diagonal row (inverse_diagonal); multigrid.hip reaches them through precond.hpp.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "multi_solve.hpp"
#include "precond.hpp"
#include "reduce_device.hpp"
#include "solve_common.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators
constexpr int kWave = 64;                 // the streaming kernels: one wavefront per workgroup, one 16-byte pair per lane

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

__device__ __forceinline__ bool usable(double v) { return v != 0.0 && isfinite(v); }

// ---- diagonal extraction: d_i = sum of row i's entries in column i, CSR order, from 0.0; dinv_i = 1.0 / d_i ----
// Validity in the same pass: d_i finite, non-zero and of d_0's sign, else atomicMin(bad_row, i).

__device__ __forceinline__ double csr_diagonal(const SlabCsr& m, int r) {
    double d = 0.0;
    for (int j = m.row_ptr[r]; j < m.row_ptr[r + 1]; ++j)
        if (m.col_idx[j] == r) d += m.values[j];
    return d;
}
__device__ __forceinline__ double ell_diagonal(const int* __restrict__ idx, const double* __restrict__ val, int rows, int width, int r) {
    double d = 0.0;
    for (int k = 0; k < width; ++k)
        if (idx[(long long)k * rows + r] == r) d += val[(long long)k * rows + r];
    return d;
}

// src: 0 = CSR, 1 = ELL planes, 2 = a plain array of n values
__device__ __forceinline__ double diagonal_at(int src, const SlabCsr& m, const int* idx, const double* val, int width, int n, int r) {
    if (src == 0) return csr_diagonal(m, r);
    if (src == 1) return ell_diagonal(idx, val, n, width, r);
    return 0.0 + val[r];
}

__global__ __launch_bounds__(256) void diagonal_inverse_kernel(int src, SlabCsr m, const int* __restrict__ idx, const double* __restrict__ val,
                                                               int width, int n, double* __restrict__ dinv, int* __restrict__ bad_row) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n) return;
    const double d0 = diagonal_at(src, m, idx, val, width, n, 0);  // row 0: a few entries, the same cached lines for every lane
    const double d = r == 0 ? d0 : diagonal_at(src, m, idx, val, width, n, r);
    if (!usable(d) || (d > 0.0) != (d0 > 0.0)) atomicMin(bad_row, r);
    dinv[r] = 1.0 / d;
}

// ---- the loop's streaming kernels (16-byte accesses, one pair per lane; the odd last row by lane 0 of workgroup 0) ----

// r = b - Ap ; z = dinv r ; p = z ; partials of r.r and r.z (at partials[blk], partials[count + blk])
template <bool kJac>
__global__ __launch_bounds__(kWave) void pcg_init_kernel(size_t n, const double* __restrict__ b, const double* __restrict__ Ap,
                                                         const double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ p,
                                                         double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (i < (n >> 1)) {
        const d2 bv = load_once(b, i), av = load_once(Ap, i);
        d2 rv, zv;
        rv.x = fma(1.0, bv.x, -1.0 * av.x);
        rv.y = fma(1.0, bv.y, -1.0 * av.y);
        if (kJac) {
            const d2 dv = load_once(dinv, i);
            zv.x = dv.x * rv.x, zv.y = dv.y * rv.y;
        } else {
            zv = rv;
        }
        store_once(r, i, rv);
        reinterpret_cast<d2*>(p)[i] = zv;  // plain: the first SpMV reads it
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
        rz = fma(rv.x, zv.x, rz), rz = fma(rv.y, zv.y, rz);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rl = fma(1.0, b[n - 1], -1.0 * Ap[n - 1]);
        const double zl = kJac ? dinv[n - 1] * rl : rl;
        r[n - 1] = rl, p[n - 1] = zl;
        rr = fma(rl, rl, rr), rz = fma(rl, zl, rz);
    }
    rr = wave_sum(rr), rz = wave_sum(rz);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr, partials[count + blockIdx.x] = rz;
}

// r = fma(-alpha, Ap, r) (unless this iteration's pAp broke down) ; z = dinv r ; partials of r.r and r.z
template <bool kJac>
__global__ __launch_bounds__(kWave) void pcg_update_r_kernel(size_t n, const PcgScalars* __restrict__ s, const double* __restrict__ Ap,
                                                             const double* __restrict__ dinv, double* __restrict__ r,
                                                             double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 av = {0.0, 0.0}, rv = {0.0, 0.0}, dv = {1.0, 1.0};
    if (live) {  // the loads before the scalars (cg_update_r_kernel has the why)
        av = load_once(Ap, i);
        rv = load_once(r, i);
        if (kJac) dv = load_once(dinv, i);
    }
    const bool update = s->skip_update == 0;
    const double alpha = s->alpha;
    double rr = 0.0, rz = 0.0;
    if (live) {
        if (update) {
            rv.x = fma(-alpha, av.x, rv.x);
            rv.y = fma(-alpha, av.y, rv.y);
            store_once(r, i, rv);
        }
        const double zx = kJac ? dv.x * rv.x : rv.x, zy = kJac ? dv.y * rv.y : rv.y;
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
        rz = fma(rv.x, zx, rz), rz = fma(rv.y, zy, rz);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double rl = r[n - 1];
        if (update) r[n - 1] = rl = fma(-alpha, Ap[n - 1], rl);
        const double zl = kJac ? dinv[n - 1] * rl : rl;
        rr = fma(rl, rl, rr), rz = fma(rl, zl, rz);
    }
    rr = wave_sum(rr), rz = wave_sum(rz);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr, partials[count + blockIdx.x] = rz;
}

// x = fma(alpha, p, x) ; p = fma(beta, p, dinv r) unless the iteration stopped. Scalars first: nothing is read when the
// iteration's pAp broke down, and r / dinv are not read in the converging iteration.
template <bool kJac>
__global__ __launch_bounds__(kWave) void pcg_update_xp_kernel(size_t n, const PcgScalars* __restrict__ s, const double* __restrict__ r,
                                                              const double* __restrict__ dinv, double* __restrict__ p, double* __restrict__ x) {
    if (s->skip_update) return;
    const bool direction = s->converged == 0 && s->breakdown == 0;
    const double alpha = s->alpha, beta = s->beta;
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < (n >> 1)) {
        d2 xv = load_once(x, i), pv = load_once(p, i);
        xv.x = fma(alpha, pv.x, xv.x);
        xv.y = fma(alpha, pv.y, xv.y);
        store_once(x, i, xv);
        if (direction) {
            d2 zv = load_once(r, i);
            if (kJac) {
                const d2 dv = load_once(dinv, i);
                zv.x = dv.x * zv.x, zv.y = dv.y * zv.y;
            }
            pv.x = fma(beta, pv.x, zv.x);
            pv.y = fma(beta, pv.y, zv.y);
            reinterpret_cast<d2*>(p)[i] = pv;  // plain: the next SpMV's neighbour loads re-use these lines
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double pl = p[n - 1];
        x[n - 1] = fma(alpha, pl, x[n - 1]);
        if (direction) p[n - 1] = fma(beta, pl, kJac ? dinv[n - 1] * r[n - 1] : r[n - 1]);
    }
}

// ---- kind "chebyshev": lambda_max, term 0 fused into the r update, the streaming step ----

// max_i sum_j |a_ij| sqrt(|dinv_i| |dinv_j|): Gershgorin's bound on D^-1/2 A D^-1/2, which has the spectrum of D^-1 A and, unlike the
// plain row sum of D^-1 A, does not move under a symmetric diagonal scaling of A. Row i is summed in storage (CSR) order from 0.0, one
// rounding per operation. The maximum of non-negative doubles is the maximum of their bit patterns as unsigned integers: a wave tree,
// then one 64-bit unsigned atomic max per wave -- independent of the order. A NaN row wins and is refused on the host.
__global__ __launch_bounds__(256) void gershgorin_kernel(int src, SlabCsr m, const int* __restrict__ idx, const double* __restrict__ val,
                                                         int width, int n, const double* __restrict__ dinv, unsigned long long* __restrict__ out) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double sum = 0.0;
    if (r < n) {
        const double di = fabs(dinv[r]);
        if (src == 0) {
            for (int j = m.row_ptr[r]; j < m.row_ptr[r + 1]; ++j) {
                const double w = sqrt(di * fabs(dinv[m.col_idx[j]]));
                sum = sum + fabs(m.values[j]) * w;
            }
        } else {
            for (int k = 0; k < width; ++k) {
                const int c = idx[(long long)k * n + r];
                if (c < 0) continue;
                const double w = sqrt(di * fabs(dinv[c]));
                sum = sum + fabs(val[(long long)k * n + r]) * w;
            }
        }
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(sum);  // sum >= +0.0, or NaN
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_down((long long)bits, off);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, bits);
}

// The residual of the stage and term 0 of the polynomial from it, in registers. kFrom 0: r = b - Ap (the initial residual, bv = b);
// 1: r = fma(-alpha, Ap, r) unless this iteration's pAp broke down; 2: r as it is (spmv_amd_precond_apply_device: r is only read).
// Then u = dinv r ; d = c0 u ; z = d. Partials: r.r at partials[blk] (kFrom 0, 1), and r.z at partials[count + blk] when term 0 is the
// whole polynomial (last != 0, degree 0).
template <int kFrom>
__global__ __launch_bounds__(kWave) void cheb_term0_kernel(size_t n, const PcgScalars* __restrict__ s, const double* __restrict__ bv,
                                                           const double* __restrict__ Ap, const double* __restrict__ dinv, double c0,
                                                           double* __restrict__ r, double* __restrict__ d, double* __restrict__ z, int last,
                                                           double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 av = {0.0, 0.0}, rv = {0.0, 0.0}, dv = {0.0, 0.0};
    if (live) {  // the loads before the scalars
        if (kFrom != 2) av = load_once(Ap, i);
        rv = load_once(kFrom == 0 ? bv : r, i);
        dv = load_once(dinv, i);
    }
    bool update = false;
    double alpha = 0.0;
    if (kFrom == 1) update = s->skip_update == 0, alpha = s->alpha;
    double rr = 0.0, rz = 0.0;
    if (live) {
        if (kFrom == 0) {
            rv.x = fma(1.0, rv.x, -1.0 * av.x);
            rv.y = fma(1.0, rv.y, -1.0 * av.y);
            store_once(r, i, rv);
        } else if (kFrom == 1 && update) {
            rv.x = fma(-alpha, av.x, rv.x);
            rv.y = fma(-alpha, av.y, rv.y);
            store_once(r, i, rv);
        }
        d2 dd;
        dd.x = c0 * (dv.x * rv.x);
        dd.y = c0 * (dv.y * rv.y);
        store_once(d, i, dd);
        reinterpret_cast<d2*>(z)[i] = dd;  // plain: the first step's SpMV reads it
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
        if (last) rz = fma(rv.x, dd.x, rz), rz = fma(rv.y, dd.y, rz);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double rl;
        if (kFrom == 0) {
            r[n - 1] = rl = fma(1.0, bv[n - 1], -1.0 * Ap[n - 1]);
        } else {
            rl = r[n - 1];
            if (kFrom == 1 && update) r[n - 1] = rl = fma(-alpha, Ap[n - 1], rl);
        }
        const double dl = c0 * (dinv[n - 1] * rl);
        d[n - 1] = dl, z[n - 1] = dl;
        rr = fma(rl, rl, rr);
        if (last) rz = fma(rl, dl, rz);
    }
    if (kFrom != 2) {
        rr = wave_sum(rr);
        if (threadIdx.x == 0) partials[blockIdx.x] = rr;
    }
    if (last) {
        rz = wave_sum(rz);
        if (threadIdx.x == 0) partials[count + blockIdx.x] = rz;
    }
}

// One step behind a SpMV that wrote w = A z: t = fma(-1, w, r) ; u = dinv t ; d = fma(g, u, h d) ; z = z + d, d and z in place.
// Nothing is read once *stop != 0 (the iteration's verdict; null: no test). last: the partials of r.z at partials[blk].
__global__ __launch_bounds__(kWave) void cheb_step_kernel(size_t n, const int* __restrict__ stop, const double* __restrict__ w,
                                                          const double* __restrict__ r, const double* __restrict__ dinv, double g, double h,
                                                          double* __restrict__ d, double* __restrict__ z, int last, double* __restrict__ partials,
                                                          int* __restrict__ work_count) {
    if (stop != nullptr && *stop != 0) return;
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    double rz = 0.0;
    if (i < (n >> 1)) {
        const d2 wv = load_once(w, i), rv = load_once(r, i), iv = load_once(dinv, i);
        d2 dd = load_once(d, i), zv = reinterpret_cast<const d2*>(z)[i];
        dd.x = fma(g, iv.x * fma(-1.0, wv.x, rv.x), h * dd.x);
        dd.y = fma(g, iv.y * fma(-1.0, wv.y, rv.y), h * dd.y);
        zv.x = zv.x + dd.x;
        zv.y = zv.y + dd.y;
        store_once(d, i, dd);
        reinterpret_cast<d2*>(z)[i] = zv;  // plain: the next SpMV reads it
        if (last) rz = fma(rv.x, zv.x, rz), rz = fma(rv.y, zv.y, rz);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rl = r[n - 1];
        const double dl = fma(g, dinv[n - 1] * fma(-1.0, w[n - 1], rl), h * d[n - 1]);
        const double zl = z[n - 1] + dl;
        d[n - 1] = dl, z[n - 1] = zl;
        if (last) rz = fma(rl, zl, rz);
    }
    if (work_count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *work_count += 1;  // one thread per launch; launches are ordered
    if (last) {
        rz = wave_sum(rz);
        if (threadIdx.x == 0) partials[blockIdx.x] = rz;
    }
}

// z = dinv r ("jacobi") or z = r ("none") with the partials of r.z: those kinds through spmv_amd_precond_apply_device.
template <bool kJac>
__global__ __launch_bounds__(kWave) void precond_apply_kernel(size_t n, const double* __restrict__ r, const double* __restrict__ dinv,
                                                              double* __restrict__ z, double* __restrict__ partials) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    double rz = 0.0;
    if (i < (n >> 1)) {
        const d2 rv = load_once(r, i);
        d2 zv = rv;
        if (kJac) {
            const d2 dv = load_once(dinv, i);
            zv.x = dv.x * rv.x, zv.y = dv.y * rv.y;
        }
        store_once(z, i, zv);
        rz = fma(rv.x, zv.x, rz), rz = fma(rv.y, zv.y, rz);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rl = r[n - 1];
        const double zl = kJac ? dinv[n - 1] * rl : rl;
        z[n - 1] = zl;
        rz = fma(rl, zl, rz);
    }
    rz = wave_sum(rz);
    if (threadIdx.x == 0) partials[blockIdx.x] = rz;
}

// The device record of a Chebyshev solve: the scalars every kind keeps, then what only this kind needs. pcg_step's steps 3 to 5 are
// handed the record's first member and reach the rest through it.
struct ChebScalars {
    PcgScalars s;
    int stop;        // the iteration's verdict (converged or broken down): the steps' skip flag
    int steps_done;  // step launches that did work
};

// ---- reductions: NV sums of `count` partials each (value v at partials[v * count ...]) in ONE launch, then the scalar step ----
// The shape of reduce_device.hpp extended to two values: slice workgroups publish their slice sums of value 0 into the stage's
// `sums`, of value 1 into its `extra` slots; the workgroup that draws the last ticket sums both and takes the step. One
// workgroup (no stage) when there are at most 1024 partials. which: 0 = initial r.r / r.z, 1 = pAp, 2 = r.r / r.z'.
// Kind "chebyshev" (s is the first member of a ChebScalars): 3 = r.r alone with the verdict, which it also writes to the stop flag;
// 4 = r.z' alone with beta, unless the verdict stopped the iteration; 5 = r.z of an application on its own (rz = the sum).

__device__ void pcg_step(PcgScalars* s, int which, const double* total, double tol, double* hist, int hist_cap) {
    if (which == 0) {
        s->b_norm = sqrt(total[0]);
        s->residual = s->b_norm;
        s->rz = total[1];
        s->pAp = s->alpha = s->beta = 0.0;
        s->iterations = s->converged = s->breakdown = s->skip_update = 0;
        if (hist_cap > 0) hist[0] = s->b_norm;
    } else if (which == 1) {
        s->pAp = total[0];
        if (usable(s->pAp)) {
            s->alpha = s->rz / s->pAp;
        } else {
            s->alpha = 0.0;
            s->skip_update = 1;
        }
    } else if (which == 2) {
        const double res = sqrt(total[0]);
        s->iterations += 1;
        s->residual = res;
        if (s->iterations < hist_cap) hist[s->iterations] = res;
        if (s->skip_update) {
            s->breakdown = 1;
        } else if (res / s->b_norm < tol) {
            s->converged = 1;
        } else if (!usable(total[1])) {
            s->breakdown = 1;
        } else {
            s->beta = total[1] / s->rz;
            s->rz = total[1];
        }
    } else if (which == 3) {
        const double res = sqrt(total[0]);
        s->iterations += 1;
        s->residual = res;
        if (s->iterations < hist_cap) hist[s->iterations] = res;
        if (s->skip_update) s->breakdown = 1;
        else if (res / s->b_norm < tol) s->converged = 1;
        reinterpret_cast<ChebScalars*>(s)->stop = (s->converged != 0 || s->breakdown != 0) ? 1 : 0;
    } else if (which == 4) {
        if (s->converged == 0 && s->breakdown == 0) {
            if (!usable(total[0])) {
                s->breakdown = 1;
            } else {
                s->beta = total[0] / s->rz;
                s->rz = total[0];
            }
        }
    } else {
        s->rz = total[0];
    }
}

template <int NV>
__global__ __launch_bounds__(kReduceBlock) void pcg_reduce_kernel(const double* __restrict__ partials, int count, int slice, int blocks,
                                                                  double* stage_base, PcgScalars* s, int which, double tol, double* hist,
                                                                  int hist_cap) {
    __shared__ double sh[kReduceBlock];
    __shared__ int s_last;
    double total[2] = {0.0, 0.0};
    if (blocks > 1) {
        const ReduceStage stage = reduce_stage_of(stage_base);
        unsigned long long* const slot[2] = {stage.sums, stage.extra};
        const int lo = (int)blockIdx.x * slice, hi = min(lo + slice, count);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            block_tree(strided_sum(partials + (long long)v * count, lo, hi), sh);
            if (threadIdx.x == 0) publish(slot[v] + blockIdx.x, sh[0]);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const unsigned drawn = __hip_atomic_fetch_add(stage.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = drawn == (unsigned)(blocks - 1) ? 1 : 0;
            if (s_last) __hip_atomic_store(stage.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (s_last == 0) return;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double acc = 0.0;
            for (int i = (int)threadIdx.x; i < blocks; i += kReduceBlock) acc += published(slot[v] + i);
            block_tree(acc, sh);
            total[v] = sh[0];
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            block_tree(strided_sum(partials + (long long)v * count, 0, count), sh);
            total[v] = sh[0];
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) pcg_step(s, which, total, tol, hist, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_pcg_stage (the
// kernels on caller data, tests/test_pcg_stages_gpu.py). dinv is not read by the "none" instantiations. ----

void launch_pcg_init(bool jac, size_t n, const double* b, const double* Ap, const double* dinv, double* r, double* p, double* partials) {
    const dim3 grid(stream_grid(n)), block(kWave);
    const int count = (int)grid.x;
    if (jac)
        hipLaunchKernelGGL(pcg_init_kernel<true>, grid, block, 0, kStream, n, b, Ap, dinv, r, p, partials, count);
    else
        hipLaunchKernelGGL(pcg_init_kernel<false>, grid, block, 0, kStream, n, b, Ap, nullptr, r, p, partials, count);
}

void launch_pcg_update_r(bool jac, size_t n, const PcgScalars* s, const double* Ap, const double* dinv, double* r, double* partials) {
    const dim3 grid(stream_grid(n)), block(kWave);
    const int count = (int)grid.x;
    if (jac)
        hipLaunchKernelGGL(pcg_update_r_kernel<true>, grid, block, 0, kStream, n, s, Ap, dinv, r, partials, count);
    else
        hipLaunchKernelGGL(pcg_update_r_kernel<false>, grid, block, 0, kStream, n, s, Ap, nullptr, r, partials, count);
}

void launch_pcg_update_xp(bool jac, size_t n, const PcgScalars* s, const double* r, const double* dinv, double* p, double* x) {
    const dim3 grid(stream_grid(n)), block(kWave);
    if (jac)
        hipLaunchKernelGGL(pcg_update_xp_kernel<true>, grid, block, 0, kStream, n, s, r, dinv, p, x);
    else
        hipLaunchKernelGGL(pcg_update_xp_kernel<false>, grid, block, 0, kStream, n, s, r, nullptr, p, x);
}

// nv sums of `count` partials each and the scalar step `which` (0: two sums, 1: one, 2: two)
void launch_pcg_reduce(const double* partials, int count, int nv, int which, double* stage, PcgScalars* s, double tol, double* hist,
                       int hist_cap) {
    int slice = 0, blocks = 0;
    reduce_geometry(count, &slice, &blocks);
    if (nv == 1)
        hipLaunchKernelGGL(pcg_reduce_kernel<1>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
    else
        hipLaunchKernelGGL(pcg_reduce_kernel<2>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
}

// ---- kind "chebyshev": the launches ----

template <int kFrom>
void launch_cheb_term0(size_t n, const PcgScalars* s, const double* b, const double* Ap, const double* dinv, double c0, double* r, double* d,
                       double* z, bool last, double* partials) {
    const dim3 grid(stream_grid(n)), block(kWave);
    hipLaunchKernelGGL(cheb_term0_kernel<kFrom>, grid, block, 0, kStream, n, s, b, Ap, dinv, c0, r, d, z, last ? 1 : 0, partials, (int)grid.x);
}

}  // namespace

// The runner of a Chebyshev step (precond.hpp, ChebRun): the loop, spmv_amd_precond_apply_device and the multigrid cycle call it.
bool spmv_amd::cheb_step(ChebRun& c, double g, double h, bool last) {
    if (c.a.partials > 0) {  // a row-lds plan: the whole step inside the SpMV launch, z' in the other vector
        ChebStep step;
        step.r = c.r, step.dinv = c.dinv, step.d = c.d, step.z_out = c.aux, step.g = g, step.h = h, step.last = last ? 1 : 0;
        step.work_count = c.work_count;
        stage_run(c.T, &StageTimers::t_spmv, [&] { (void)launch_stencil5_cheb_step(*c.a.view, *c.a.plan, c.z, step, c.partials, c.stop, kStream); });
        double* const t = c.z;
        c.z = c.aux, c.aux = t;
        if (last) c.rz_partials = c.partials, c.rz_count = c.a.partials;
        return true;
    }
    bool ok = true;
    stage_run(c.T, &StageTimers::t_spmv, [&] {
        if (c.a.csr) {
            launch_csr_spmv(*c.a.view, c.z, c.aux, 1.0, c.a.csr_variant, kStream);
        } else if (c.a.plan7 != nullptr) {
            (void)launch_stencil7_spmv(*c.a.view, *c.a.plan7, c.z, c.aux, 1.0, nullptr, c.stop, false, kStream);
        } else if (c.a.plan != nullptr) {
            (void)launch_stencil5_spmv(*c.a.view, *c.a.plan, c.z, c.aux, 1.0, nullptr, c.stop, false, kStream);
        } else if (c.a.op->run_device(c.z, c.aux) != 0) {
            fprintf(stderr, "[PCG] operator '%s': run_device failed\n", c.a.op->name);
            ok = false;
        }
    });
    if (!ok) return false;
    stage_run(c.T, &StageTimers::t_blas, [&] {
        hipLaunchKernelGGL(cheb_step_kernel, dim3(stream_grid(c.n)), dim3(kWave), 0, kStream, c.n, c.stop, c.aux, c.r, c.dinv, g, h, c.d, c.z,
                           last ? 1 : 0, c.partials, c.work_count);
    });
    if (last) c.rz_partials = c.partials, c.rz_count = (int)stream_grid(c.n);
    return true;
}

bool spmv_amd::cheb_steps(ChebRun& c, int degree, const double* coef, bool report) {
    for (int k = 1; k <= degree; ++k)
        if (!cheb_step(c, coef[2 * k], coef[2 * k - 1], report && k == degree)) return false;
    return true;
}

namespace {

// Steps 1 .. degree of m's polynomial behind a term 0 that left d and z in c -- and, at degree 0, the r.z partials behind its r.r ones.
bool cheb_after_term0(const SpmvAmdPrecond* m, ChebRun& c) {
    c.rz_partials = c.partials + stream_grid(c.n), c.rz_count = (int)stream_grid(c.n);
    return cheb_steps(c, m->degree, m->coef, true);
}

// ---- workspace: kept between calls (like cg_solve_device's), released with it ----
struct PcgWorkspace {
    int n = 0, device = -1;
    double *x = nullptr, *b = nullptr, *r = nullptr, *p = nullptr, *Ap = nullptr;
    double* partials = nullptr;  // max(the fused SpMV's slots, 2 x streaming workgroups)
    double* stage = nullptr;     // reduce_scratch_alloc()
    PcgScalars* s = nullptr;
    double* hist = nullptr;
    int hist_cap = 0;
    long long partial_cap = 0;
    double *cd = nullptr, *cz = nullptr, *cz2 = nullptr;  // kind "chebyshev" only: d, z and the fused step's second z
    void release() {
        device_release(cd);
        device_release(cz);
        device_release(cz2);
        device_release(x);
        device_release(b);
        device_release(r);
        device_release(p);
        device_release(Ap);
        device_release(partials);
        device_release(stage);
        device_release(s);
        device_release(hist);
        n = 0, device = -1, hist_cap = 0, partial_cap = 0;
    }
};
PcgWorkspace g_pcg;
std::vector<double> g_pcg_history;  // of the last preconditioned solve
int g_mg_cycles = 0;                // V-cycles of the last solve's loop (kind "multigrid"; the LAB build hands it out)
int g_cheb_step_launches = 0;       // Chebyshev step launches of its loop that did work (the LAB build hands it out)

bool fail(const char* what) {
    fprintf(stderr, "[PCG] %s\n", what);
    return false;
}

bool ensure_workspace(int n, int device, long long partial_cap, int hist_cap) {
    PcgWorkspace& w = g_pcg;
    if (w.x != nullptr && (w.n != n || w.device != device || w.partial_cap < partial_cap)) w.release();
    if (w.x == nullptr) {
        const size_t need = 5 * (size_t)n * sizeof(double) + (size_t)partial_cap * sizeof(double) + (size_t)hist_cap * sizeof(double) +
                            ((size_t)64 << 20);
        char what[32];
        snprintf(what, sizeof what, "%d rows", n);
        if (!device_has_room(need, "PCG", what)) return false;
        w.x = device_try_alloc<double>((size_t)n);
        w.b = device_try_alloc<double>((size_t)n);
        w.r = device_try_alloc<double>((size_t)n);
        w.p = device_try_alloc<double>((size_t)n);
        w.Ap = device_try_alloc<double>((size_t)n);
        w.partials = device_try_alloc<double>((size_t)partial_cap);
        w.s = reinterpret_cast<PcgScalars*>(device_try_alloc<ChebScalars>(1));  // the Chebyshev loop's record begins with the common one
        if (!w.x || !w.b || !w.r || !w.p || !w.Ap || !w.partials || !w.s) {
            w.release();
            return fail("the workspace could not be allocated: refused");
        }
        w.stage = reduce_scratch_alloc();
        w.n = n, w.device = device, w.partial_cap = partial_cap;
    }
    if (!grow_history(w.hist, w.hist_cap, hist_cap)) return fail("the history could not be allocated: refused");
    return true;
}

// d, z, z' of the Chebyshev loop, next to a workspace ensure_workspace() has made; sized against free memory like the rest
bool ensure_cheb_workspace(int n) {
    PcgWorkspace& w = g_pcg;
    if (w.cd != nullptr) return true;
    char what[48];
    snprintf(what, sizeof what, "%d rows (chebyshev)", n);
    if (!device_has_room(3 * (size_t)n * sizeof(double) + ((size_t)64 << 20), "PCG", what)) return false;
    w.cd = device_try_alloc<double>((size_t)n);
    w.cz = device_try_alloc<double>((size_t)n);
    w.cz2 = device_try_alloc<double>((size_t)n);
    if (!w.cd || !w.cz || !w.cz2) {
        device_release(w.cd);
        device_release(w.cz);
        device_release(w.cz2);
        return fail("the Chebyshev vectors could not be allocated: refused");
    }
    return true;
}

int kind_of(const char* kind) {
    if (kind == nullptr) return -1;
    if (!strcmp(kind, "none")) return kNone;
    if (!strcmp(kind, "jacobi")) return kJacobi;
    return -1;
}

// The diagonal pass over a diagonal source: dinv on the device, or null -- no device memory, or a row at fault: the first one is named on
// stderr behind `who` (the only place of that sentence) and stored in *bad_row where that is not null.
double* inverse_diagonal(int src, const SlabCsr& m, const int* idx, const double* val, int width, int n, const char* who, int* bad_row) {
    double* dinv = device_try_alloc<double>((size_t)n);
    int* d_bad = device_try_alloc<int>(1);
    if (dinv == nullptr || d_bad == nullptr) {
        device_release(dinv);
        device_release(d_bad);
        fail("no device memory for the inverse diagonal");
        return nullptr;
    }
    const int none = INT_MAX;
    upload(d_bad, &none, 1);
    hipLaunchKernelGGL(diagonal_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, kStream, src, m, idx, val, width, n, dinv, d_bad);
    HIP_CHECK(hipGetLastError());
    int bad = none;
    download(&bad, d_bad, 1);  // synchronises
    device_release(d_bad);
    if (bad != none) {
        device_release(dinv);
        if (bad_row != nullptr) *bad_row = bad;
        fprintf(stderr, "[PCG] %s: the diagonal entry of row %d is zero, not finite or of the other sign than row 0's: refused\n", who, bad);
        return nullptr;
    }
    return dinv;
}

// The validity pass over a diagonal source; returns the preconditioner or null (*bad_row set when a row is at fault).
SpmvAmdPrecond* make_jacobi(int src, const SlabCsr& m, const int* idx, const double* val, int width, int n, int* bad_row) {
    double* dinv = inverse_diagonal(src, m, idx, val, width, n, "jacobi", bad_row);
    if (dinv == nullptr) return nullptr;
    SpmvAmdPrecond* pm = new SpmvAmdPrecond();
    pm->kind = kJacobi;
    pm->n = n;
    pm->dinv = dinv;
    return pm;
}

// lambda_max of D^-1 A by gershgorin_kernel
double gershgorin_bound(int src, const SlabCsr& m, const int* idx, const double* val, int width, int rows, const double* dinv) {
    unsigned long long* d_bits = device_alloc<unsigned long long>(1);
    const unsigned long long zero = 0;
    upload(d_bits, &zero, 1);
    hipLaunchKernelGGL(gershgorin_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, kStream, src, m, idx, val, width, rows, dinv, d_bits);
    HIP_CHECK(hipGetLastError());
    unsigned long long bits = 0;
    download(&bits, d_bits, 1);  // synchronises
    device_release(d_bits);
    double bound = 0.0;
    memcpy(&bound, &bits, sizeof bound);
    return bound;
}

}  // namespace

namespace spmv_amd {
void release_pcg_workspace_locked() { g_pcg.release(); }
}  // namespace spmv_amd

extern "C" SpmvAmdPrecond* spmv_amd_precond_create(SpmvOperator* op, const char* kind, int* bad_row) {
    if (bad_row != nullptr) *bad_row = -1;
    const int k = kind_of(kind);
    if (k < 0) {
        fprintf(stderr, "[PCG] unknown preconditioner kind '%s' (none, jacobi)\n", kind ? kind : "(null)");
        return nullptr;
    }
    if (op == nullptr) return fail("null operator"), nullptr;
    DiagonalSource d;
    if (!creation_source(op, "", "one of this library's: pass its diagonal to spmv_amd_precond_create_from_diagonal", 0, &d)) return nullptr;
    SpmvAmdPrecond* pm = nullptr;
    if (k == kNone) {
        pm = new SpmvAmdPrecond();
        pm->kind = kNone;
        pm->n = d.rows;
    } else {
        pm = make_jacobi(d.kind == DiagonalSource::Csr ? 0 : 1, d.csr, d.idx, d.val, d.width, d.rows, bad_row);
        if (pm == nullptr) return nullptr;
    }
    pm->owner = d.owner;
    pm->generation = d.generation;
    return pm;
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_from_diagonal(const double* d_diag, int n, int* bad_row) {
    if (bad_row != nullptr) *bad_row = -1;
    if (d_diag == nullptr) return fail("null diagonal"), nullptr;
    if (n < 1) return fail("n < 1"), nullptr;
    return make_jacobi(2, SlabCsr{}, nullptr, d_diag, 0, n, bad_row);
}

// The coefficients of the degree-k Chebyshev polynomial on [lmin, lmax], in the order and with the operations api.h states (the file is
// compiled with -ffp-contract=off: one rounding per operation).
void spmv_amd::chebyshev_coefficients(int degree, double lmin, double lmax, double* coef) {
    const double theta = 0.5 * (lmax + lmin);
    const double delta = 0.5 * (lmax - lmin);
    const double sigma = theta / delta;
    coef[0] = 1.0 / theta;
    double rho = 1.0 / sigma;
    for (int k = 1; k <= degree; ++k) {
        const double rho_next = 1.0 / (2.0 * sigma - rho);
        coef[2 * k - 1] = rho_next * rho;
        coef[2 * k] = 2.0 * rho_next / delta;
        rho = rho_next;
    }
}

// pcg.hip's set-up passes, the creators' operator check and term 0 for multigrid.hip (precond.hpp)
namespace spmv_amd {
double* inverse_diagonal_of_csr(const SlabCsr& m, int n, const char* who, int* bad_row) {
    return inverse_diagonal(0, m, nullptr, nullptr, 0, n, who, bad_row);
}
double gershgorin_of_csr(const SlabCsr& m, int n, const double* dinv) { return gershgorin_bound(0, m, nullptr, nullptr, 0, n, dinv); }
void launch_cheb_term0_apply(size_t n, const double* r, const double* dinv, double c0, double* d, double* z) {
    launch_cheb_term0<2>(n, nullptr, nullptr, nullptr, dinv, c0, const_cast<double*>(r), d, z, false, nullptr);
}
bool creation_source(const SpmvOperator* op, const char* label, const char* not_ours, int stencil_dim, DiagonalSource* d) {
    *d = diagonal_source_of(op);
    bool ours = d->owner != nullptr;
    if (stencil_dim == 2)
        ours = ours && d->kind == DiagonalSource::Csr && op->name != nullptr &&
               (strcmp(op->name, "stencil5-csr") == 0 || strcmp(op->name, "stencil5-halo-mgpu") == 0);
    else if (stencil_dim == 3)
        ours = ours && d->kind == DiagonalSource::Csr && op->name != nullptr && strcmp(op->name, "stencil7-csr") == 0;
    if (!ours) {
        fprintf(stderr, "[PCG] %soperator '%s' is not %s\n", label, op->name ? op->name : "?", not_ours);
        return false;
    }
    if (!d->ready) {
        fprintf(stderr, "[PCG] operator '%s' used before init\n", op->name);
        return false;
    }
    if (stencil_dim == 0 && d->rows != d->cols) {  // a stencil-only creator has a stricter test of its own behind this
        fprintf(stderr, "[PCG] operator '%s' holds a %d x %d matrix: a square one is required\n", op->name, d->rows, d->cols);
        return false;
    }
    return true;
}
}  // namespace spmv_amd

// What every entry point that takes (op, m) checks of the pair before any HIP call; d: the operator's storage view (precond.hpp).
bool spmv_amd::precond_matches(const SpmvOperator* op, const SpmvAmdPrecond* m, const DiagonalSource& d) {
    if (m->owner == nullptr) return true;  // made from a caller's diagonal: no operator to belong to
    if (m->owner != d.owner) return fail("the preconditioner was made from another operator: refused");
    if (m->generation != d.generation)
        return fail("the preconditioner was made before the operator was last initialised or freed: refused");
    if (!d.ready) {
        fprintf(stderr, "[PCG] operator '%s' used before init\n", op->name);
        return false;
    }
    return true;
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_chebyshev(SpmvOperator* op, int degree, double lambda_min, double lambda_max, int* bad_row) {
    // argument checks: all before the first HIP call
    if (bad_row != nullptr) *bad_row = -1;
    if (op == nullptr) return fail("null operator"), nullptr;
    if (degree < 0 || degree > kChebMaxDegree) {
        fprintf(stderr, "[PCG] chebyshev: degree %d is outside 0..%d: refused\n", degree, kChebMaxDegree);
        return nullptr;
    }
    if (!isfinite(lambda_min) || !isfinite(lambda_max)) return fail("chebyshev: a bound that is not finite: refused"), nullptr;
    if (lambda_min > 0.0 && lambda_max > 0.0 && !(lambda_min < lambda_max)) return fail("chebyshev: lambda_min >= lambda_max: refused"), nullptr;
    DiagonalSource d;
    if (!creation_source(op, "chebyshev: ", "one of this library's: refused", 0, &d)) return nullptr;
    const int src = d.kind == DiagonalSource::Csr ? 0 : 1;
    SpmvAmdPrecond* pm = make_jacobi(src, d.csr, d.idx, d.val, d.width, d.rows, bad_row);
    if (pm == nullptr) return nullptr;
    pm->kind = kChebyshev;
    pm->degree = degree;
    pm->owner = d.owner;
    pm->generation = d.generation;
    double lmax = lambda_max;
    if (!(lmax > 0.0)) {
        lmax = gershgorin_bound(src, d.csr, d.idx, d.val, d.width, d.rows, pm->dinv);
    }
    const double lmin = lambda_min > 0.0 ? lambda_min : lmax / 30.0;
    if (!isfinite(lmax) || !isfinite(lmin) || !(lmin > 0.0) || !(lmin < lmax)) {
        fprintf(stderr, "[PCG] chebyshev: the interval [%g, %g] is not 0 < lambda_min < lambda_max, both finite: refused\n", lmin, lmax);
        spmv_amd_precond_destroy(pm);
        return nullptr;
    }
    pm->lambda_min = lmin, pm->lambda_max = lmax;
    chebyshev_coefficients(degree, lmin, lmax, pm->coef);
    return pm;
}

extern "C" int spmv_amd_precond_chebyshev_info(const SpmvAmdPrecond* m, int* degree, double* lambda_min, double* lambda_max,
                                               double* coefficients, int cap) {
    if (m == nullptr || m->kind != kChebyshev) return 0;
    if (degree != nullptr) *degree = m->degree;
    if (lambda_min != nullptr) *lambda_min = m->lambda_min;
    if (lambda_max != nullptr) *lambda_max = m->lambda_max;
    const int count = 1 + 2 * m->degree;
    for (int i = 0; i < count && i < cap && coefficients != nullptr; ++i) coefficients[i] = m->coef[i];
    return count;
}

extern "C" int spmv_amd_precond_apply_device(SpmvOperator* op, const SpmvAmdPrecond* m, const double* d_r, double* d_z, double* rz) {
    // argument checks: all before the first HIP call
    if (op == nullptr || m == nullptr || d_r == nullptr || d_z == nullptr) return fail("null argument"), 1;
    if ((((uintptr_t)d_r) & 15) != 0 || (((uintptr_t)d_z) & 15) != 0) return fail("apply: a vector is not 16-byte aligned: refused"), 1;
    const size_t n = (size_t)m->n;
    {
        const uintptr_t a = (uintptr_t)d_r, b = (uintptr_t)d_z, bytes = n * sizeof(double);
        if (a < b + bytes && b < a + bytes) return fail("apply: d_z overlaps d_r: refused"), 1;
    }
    const DiagonalSource d = diagonal_source_of(op);
    if (!precond_matches(op, m, d)) return 1;
    const bool jac = m->kind == kJacobi, cheb = m->kind == kChebyshev, mg = m->kind == kMultigrid;  // which application runs below
    if ((cheb || mg) && (op->run_device == nullptr || d.owner == nullptr || d.rows != m->n || d.cols != m->n))
        return fail("apply: the operator is not the initialised square one the preconditioner was made from: refused"), 1;

    CgWorkspaceScope scope;
    const int vec_count = (int)stream_grid(n);
    ChebRun c;  // kind "chebyshev": the application on temporaries of this call
    if (cheb) c.a = cheb_spmv_of(op);
    const long long slots = 2LL * vec_count > c.a.partials ? 2LL * vec_count : (long long)c.a.partials;
    double* partials = device_try_alloc<double>((size_t)slots);
    ChebScalars* cs = device_try_alloc<ChebScalars>(1);
    double* stage = reduce_scratch_alloc();
    double *cd = nullptr, *cz2 = nullptr, *cw = nullptr;
    const bool fused = c.a.partials > 0;
    bool ok = partials != nullptr && cs != nullptr;
    if (ok && cheb) {
        cd = device_try_alloc<double>(n);
        if (m->degree > 0) (fused ? cz2 : cw) = device_try_alloc<double>(n);
        ok = cd != nullptr && (m->degree == 0 || cz2 != nullptr || cw != nullptr);
    }
    int rc = 0;
    if (!ok) {
        rc = 1;
        fail("apply: the work vectors could not be allocated: refused");
    } else {
        HIP_CHECK(hipMemsetAsync(cs, 0, sizeof(ChebScalars), kStream));
        Applied out;  // null z: refused
        if (mg) {
            out = mg_cycle(m->mg, d_r, nullptr);
            HIP_CHECK(hipMemcpyAsync(d_z, out.z, n * sizeof(double), hipMemcpyDeviceToDevice, kStream));
        } else if (cheb) {
            // the fused step alternates between two z vectors: start where an application of this degree ends in d_z
            c.n = n, c.r = d_r, c.dinv = m->dinv, c.d = cd, c.partials = partials;
            c.z = fused && (m->degree & 1) ? cz2 : d_z;
            c.aux = !fused ? cw : c.z == d_z ? cz2 : d_z;
            launch_cheb_term0<2>(n, &cs->s, nullptr, nullptr, m->dinv, m->coef[0], const_cast<double*>(d_r), cd, c.z, m->degree == 0, partials);
            if (cheb_after_term0(m, c)) {
                if (c.z == d_z) out.z = d_z, out.rz_partials = c.rz_partials, out.rz_count = c.rz_count;
                else fail("apply: internal error, the result is not in d_z");
            }
        } else {
            const dim3 grid((unsigned)vec_count), block(kWave);
            if (jac) hipLaunchKernelGGL(precond_apply_kernel<true>, grid, block, 0, kStream, n, d_r, m->dinv, d_z, partials);
            else hipLaunchKernelGGL(precond_apply_kernel<false>, grid, block, 0, kStream, n, d_r, nullptr, d_z, partials);
            out.z = d_z, out.rz_partials = partials, out.rz_count = vec_count;
        }
        if (out.z == nullptr) {
            rc = 1;
        } else {
            launch_pcg_reduce(out.rz_partials, out.rz_count, 1, 5, stage, &cs->s, 0.0, nullptr, 0);
            HIP_CHECK(hipGetLastError());
            PcgScalars h{};
            download(&h, &cs->s, 1);  // synchronises
            if (rz != nullptr) *rz = h.rz;
        }
    }
    HIP_CHECK(hipDeviceSynchronize());
    device_release(partials);
    device_release(cs);
    device_release(stage);
    device_release(cd);
    device_release(cz2);
    device_release(cw);
    return rc;
}

extern "C" void spmv_amd_precond_destroy(SpmvAmdPrecond* m) {
    if (m == nullptr) return;
    mg_destroy(m->mg);
    device_release(m->dinv);
    delete m;
}

extern "C" const char* spmv_amd_precond_kind(const SpmvAmdPrecond* m) {
    if (m == nullptr) return "invalid";
    return m->kind == kMultigrid ? "multigrid" : m->kind == kChebyshev ? "chebyshev" : m->kind == kJacobi ? "jacobi" : "none";
}

extern "C" int spmv_amd_precond_inverse_diagonal(const SpmvAmdPrecond* m, double* out, int n) {
    if (m == nullptr || out == nullptr) return fail("null argument"), 1;
    if (m->kind == kNone) return fail("kind 'none' has no inverse diagonal"), 1;
    if (n != m->n) {
        fprintf(stderr, "[PCG] the preconditioner has %d values, %d asked for\n", m->n, n);
        return 1;
    }
    HIP_CHECK(hipStreamSynchronize(kStream));
    download(out, m->dinv, (size_t)n);
    return 0;
}

namespace {

// ---- the loop's per-kind units ----
// What the units of one solve share: the solve's arguments, its workspace and timers, and what the host knows of its state.
struct PcgLoop {
    const SpmvOperator* op;
    const SpmvAmdPrecond* m;
    size_t n;
    int vec_count;  // partials of a streaming kernel
    double tol;
    ChebSpmv a;     // how the operator runs A z for a Chebyshev step
    PcgWorkspace& w;
    StageTimers& T;
    bool failed = false;          // the operator's run_device refused
    PcgScalars h{};               // the host's copy of the device scalars
    int cycles = 0;               // kind "multigrid": V-cycles of the loop
    int* step_counter = nullptr;  // kind "chebyshev": the device count of its loop's step launches that did work

    ChebScalars* record() const { return reinterpret_cast<ChebScalars*>(w.s); }
    template <class F>
    void blas(F&& launch) { T.run(&T.t_blas, launch); }
    void reduce_at(const double* partials, int count, int nv, int which) {
        T.run(&T.t_red, [&] { launch_pcg_reduce(partials, count, nv, which, w.stage, w.s, tol, w.hist, w.hist_cap); });
    }
    void reduce(int count, int nv, int which) { reduce_at(w.partials, count, nv, which); }
    template <class F>
    void spmv(F&& launch) { T.run(&T.t_spmv, launch); }
    void run_A(const double* in, double* out) {  // out = A in through the vtable
        if (op->run_device(in, out) != 0) {
            fprintf(stderr, "[PCG] operator '%s': run_device failed\n", op->name);
            failed = true;
        }
    }
    // z0 = M^-1 r0 is the first direction
    void first_direction(const double* z0) { HIP_CHECK(hipMemcpyAsync(w.p, z0, n * sizeof(double), hipMemcpyDeviceToDevice, kStream)); }
};

// One unit per kind. first: everything before the loop -- r0 = b - A x0, ||r0||, z0 = M^-1 r0, r0.z0, p0 = z0. next: what lies between
// the sum of p.Ap and the x / p update -- r -= alpha Ap, ||r|| with the verdict, z = M^-1 r, beta -- and returns the vector the x / p
// update reads (with dinv inside the kernel where jac is set), or null when the operator's run_device refused.
struct PcgKind {
    bool jac;
    bool vectors;  // d, z and z' join the workspace (ensure_cheb_workspace)
    void (*first)(PcgLoop&);
    const double* (*next)(PcgLoop&);
};

// "none" / "jacobi": z stays in the kernels' registers, r.r and r.z are summed in one launch
template <bool kJac>
void plain_first(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    L.spmv([&] { L.run_A(w.x, w.Ap); });
    L.blas([&] { launch_pcg_init(kJac, L.n, w.b, w.Ap, L.m->dinv, w.r, w.p, w.partials); });
    L.reduce(L.vec_count, 2, 0);
}
template <bool kJac>
const double* plain_next(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    L.blas([&] { launch_pcg_update_r(kJac, L.n, w.s, w.Ap, L.m->dinv, w.r, w.partials); });
    L.reduce(L.vec_count, 2, 2);
    return w.r;
}

// "chebyshev": term 0 rides on the r update; the steps behind it test the verdict on the device (first: no flag, none is up yet)
const double* cheb_steps_and_rz(PcgLoop& L, const int* stop, int* work_count, int which) {
    PcgWorkspace& w = L.w;
    ChebRun c;
    c.a = L.a, c.n = L.n, c.r = w.r, c.dinv = L.m->dinv, c.d = w.cd, c.z = w.cz, c.aux = L.a.partials > 0 ? w.cz2 : w.Ap;
    c.partials = w.partials, c.stop = stop, c.work_count = work_count, c.T = &L.T;
    if (L.failed || !cheb_after_term0(L.m, c)) return L.failed = true, nullptr;
    L.reduce_at(c.rz_partials, c.rz_count, 1, which);
    return c.z;
}
void cheb_first(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    HIP_CHECK(hipMemsetAsync(L.record(), 0, sizeof(ChebScalars), kStream));
    L.step_counter = &L.record()->steps_done;
    L.spmv([&] { L.run_A(w.x, w.Ap); });
    L.blas([&] { launch_cheb_term0<0>(L.n, w.s, w.b, w.Ap, L.m->dinv, L.m->coef[0], w.r, w.cd, w.cz, L.m->degree == 0, w.partials); });
    L.reduce(L.vec_count, 1, 0);
    const double* const z0 = cheb_steps_and_rz(L, nullptr, nullptr, 5);
    if (z0 != nullptr) L.first_direction(z0);
}
const double* cheb_next(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    L.blas([&] { launch_cheb_term0<1>(L.n, w.s, nullptr, w.Ap, L.m->dinv, L.m->coef[0], w.r, w.cd, w.cz, L.m->degree == 0, w.partials); });
    L.reduce(L.vec_count, 1, 3);  // r.r and the verdict: the steps test it on the device
    return cheb_steps_and_rz(L, &L.record()->stop, L.step_counter, 4);
}

// "multigrid": the "none" r update, then one V-cycle on r (multigrid.hip) unless the host reads a verdict that ends the solve
const double* mg_cycle_and_rz(PcgLoop& L, int which) {
    const Applied cycle = mg_cycle(L.m->mg, L.w.r, &L.T);
    L.reduce_at(cycle.rz_partials, cycle.rz_count, 1, which);
    return cycle.z;
}
void mg_first(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    HIP_CHECK(hipMemsetAsync(L.record(), 0, sizeof(ChebScalars), kStream));
    L.spmv([&] { L.run_A(w.x, w.Ap); });
    L.blas([&] { launch_pcg_init(false, L.n, w.b, w.Ap, nullptr, w.r, w.p, w.partials); });
    L.reduce(L.vec_count, 1, 0);
    if (!L.failed) L.first_direction(mg_cycle_and_rz(L, 5));
}
const double* mg_next(PcgLoop& L) {
    PcgWorkspace& w = L.w;
    L.blas([&] { launch_pcg_update_r(false, L.n, w.s, w.Ap, nullptr, w.r, w.partials); });
    L.reduce(L.vec_count, 1, 3);  // r.r and the verdict
    download(&L.h, w.s, 1);       // the host reads it first: the converging iteration runs no cycle
    if (L.h.converged || L.h.breakdown) return mg_result_vector(L.m->mg);
    ++L.cycles;
    return mg_cycle_and_rz(L, 4);
}

PcgKind pcg_kind_of(const SpmvAmdPrecond* m) {
    if (m->kind == kMultigrid) return {false, false, mg_first, mg_next};
    if (m->kind == kChebyshev) return {false, true, cheb_first, cheb_next};
    if (m->kind == kJacobi) return {true, false, plain_first<true>, plain_next<true>};
    return {false, false, plain_first<false>, plain_next<false>};
}

}  // namespace

extern "C" int spmv_amd_pcg_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, const double* b, double* x,
                                         const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (op == nullptr || mat == nullptr || m == nullptr || b == nullptr || x == nullptr || config == nullptr || stats == nullptr)
        return fail("null argument"), 1;
    if (op->run_device == nullptr) {
        fprintf(stderr, "[PCG] operator '%s' does not support the device-native interface\n", op->name ? op->name : "?");
        return 1;
    }
    if (config->max_iters < 0) return fail("max_iters < 0"), 1;
    const DiagonalSource d = diagonal_source_of(op);
    if (d.owner != nullptr) {
        if (!d.ready) {
            fprintf(stderr, "[PCG] operator '%s' used before init\n", op->name);
            return 1;
        }
        if (d.rows != d.cols || mat->rows != d.rows) {
            fprintf(stderr, "[PCG] the operator holds a %d x %d matrix, mat->rows = %d: a square system of that size is required\n", d.rows,
                    d.cols, mat->rows);
            return 1;
        }
    }
    if (mat->rows < 1) return fail("mat->rows < 1"), 1;
    if (m->n != mat->rows) {
        fprintf(stderr, "[PCG] the preconditioner is for %d rows, mat->rows = %d\n", m->n, mat->rows);
        return 1;
    }
    if (!precond_matches(op, m, d)) return 1;
    const int n = mat->rows;
    const CGConfig cfg = *config;
    const PcgKind kind = pcg_kind_of(m);

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const FusedSpmv f = fused_spmv_of(op);
    const bool fused = f.launch != nullptr && f.partials > 0;
    const int vec_count = (int)stream_grid((size_t)n);
    const ChebSpmv a = kind.vectors ? cheb_spmv_of(op) : ChebSpmv{};
    long long partial_cap = 2LL * vec_count > f.partials ? 2LL * vec_count : (long long)f.partials;
    if (a.partials > partial_cap) partial_cap = a.partials;
    if (!ensure_workspace(n, device, partial_cap, cfg.max_iters + 1)) return 1;
    if (kind.vectors && !ensure_cheb_workspace(n)) return 1;
    PcgWorkspace& w = g_pcg;
    upload(w.b, b, (size_t)n);
    upload(w.x, x, (size_t)n);

    StageTimers T(cfg.enable_detailed_timers != 0, kStream);
    PcgLoop L{op, m, (size_t)n, vec_count, cfg.tolerance, a, w, T};
    PcgScalars& h = L.h;

    T.total.begin(kStream);
    kind.first(L);
    download(&h, w.s, 1);
    if (cfg.verbose >= 1)
        printf("[PCG-DEVICE] Initial residual: %e (preconditioner %s)\n", h.b_norm, spmv_amd_precond_kind(m));
    for (int it = 0; it < cfg.max_iters && !L.failed && !h.converged && !h.breakdown; ++it) {
        int pap_count = vec_count;
        L.spmv([&] {  // Ap = A p with the p.Ap partials
            if (fused) {
                pap_count = f.launch(w.p, w.Ap, w.partials, nullptr, false, nullptr, kStream);
            } else {
                L.run_A(w.p, w.Ap);
                launch_dot_partials((size_t)n, w.p, w.Ap, w.partials, kStream);
            }
        });
        if (L.failed) break;
        L.reduce(pap_count, 1, 1);  // alpha = rz / pAp
        const double* const z = kind.next(L);
        if (z == nullptr) break;
        L.blas([&] { launch_pcg_update_xp(kind.jac, (size_t)n, w.s, z, m->dinv, w.p, w.x); });
        download(&h, w.s, 1);  // synchronises: the stopping test
        if (cfg.verbose >= 2)
            printf("[PCG-DEVICE] Iter %3d: residual = %e (rel = %e)\n", h.iterations, h.residual, h.residual / h.b_norm);
    }
    T.total.end(kStream);
    const double total_ms = T.total.elapsed_ms();
    HIP_CHECK(hipGetLastError());
    download(x, w.x, (size_t)n);
    const int count = h.iterations + 1 < w.hist_cap ? h.iterations + 1 : w.hist_cap;
    g_pcg_history.assign((size_t)count, 0.0);
    download(g_pcg_history.data(), w.hist, (size_t)count);
    g_mg_cycles = L.cycles;
    g_cheb_step_launches = 0;
    if (L.step_counter != nullptr) download(&g_cheb_step_launches, L.step_counter, 1);
    if (L.failed) return 1;

    fill_device_stats(stats, h.iterations, h.converged != 0, h.residual, h.b_norm, cfg, total_ms, T.t_spmv, T.t_blas, T.t_red);
    solution_checksums(x, n, &stats->solution_sum, &stats->solution_norm);
    if (cfg.verbose >= 1) {
        if (h.breakdown) printf("[PCG-DEVICE] Breakdown in iteration %d (pAp or r.z zero or not finite)\n", h.iterations);
        printf("[PCG-DEVICE] Converged: %s\n", stats->converged ? "YES" : "NO");
        printf("[PCG-DEVICE] Iterations: %d\n", stats->iterations);
        printf("[PCG-DEVICE] Final residual: %e\n", stats->residual_norm);
        printf("[PCG-DEVICE] Time breakdown:\n");
        printf("     Total:      %.3f ms\n", stats->time_total_ms);
        printf("     SpMV:       %.3f ms\n", stats->time_spmv_ms);
        printf("     BLAS1:      %.3f ms\n", stats->time_blas1_ms);
        printf("     Reductions: %.3f ms\n", stats->time_reductions_ms);
    }
    return 0;
}

extern "C" int spmv_amd_pcg_last_history(double* out, int cap) {
    return copy_history(g_pcg_history, out, cap);
}

extern "C" void spmv_amd_pcg_release_workspace(void) { spmv_amd::release_cg_workspace(); }

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_pcg_last_step_launches(void) { return g_cheb_step_launches; }
extern "C" int spmv_amd_pcg_last_multigrid_cycles(void) { return g_mg_cycles; }

// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_pcg_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdPcgScalars) == sizeof(PcgScalars) && offsetof(SpmvAmdPcgScalars, b_norm) == offsetof(PcgScalars, b_norm) &&
                  offsetof(SpmvAmdPcgScalars, iterations) == offsetof(PcgScalars, iterations) &&
                  offsetof(SpmvAmdPcgScalars, skip_update) == offsetof(PcgScalars, skip_update),
              "lab.h's scalar record is the device record, field for field");

extern "C" int spmv_amd_pcg_stage(const char* stage, const char* kind, SpmvAmdPcgStageArgs* a, SpmvAmdPcgScalars* scalars) {
    // argument checks: all before the first HIP call. 16: a vector the streaming kernels read or write in 16-byte pairs; 8: an array
    // of doubles read or written one at a time
    auto refuse = [&](const char* what) { return stage_fail("PCG", stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer("PCG", stage, name, ptr, align); };
    enum { kInit, kUpdateR, kUpdateXp, kReduce } st;
    if (stage == nullptr) return refuse("no stage named (init, update_r, update_xp, reduce)"), 1;
    if (!strcmp(stage, "init")) st = kInit;
    else if (!strcmp(stage, "update_r")) st = kUpdateR;
    else if (!strcmp(stage, "update_xp")) st = kUpdateXp;
    else if (!strcmp(stage, "reduce")) st = kReduce;
    else return refuse("unknown stage (init, update_r, update_xp, reduce)"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    bool jac = false;
    if (st != kReduce) {
        const int k = kind_of(kind);
        if (k < 0) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
        jac = k == kJacobi;
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
        if (jac && !pointer("dinv", a->dinv, 16)) return 1;
    }
    if (st != kInit && scalars == nullptr) return refuse("null scalar record"), 1;
    if (st == kInit) {
        if (!pointer("b", a->b, 16) || !pointer("Ap", a->Ap, 16) || !pointer("r", a->r, 16) ||
            !pointer("p", a->p, 16) || !pointer("partials", a->partials, 8))
            return 1;
    } else if (st == kUpdateR) {
        if (!pointer("Ap", a->Ap, 16) || !pointer("r", a->r, 16) || !pointer("partials", a->partials, 8)) return 1;
    } else if (st == kUpdateXp) {
        if (!pointer("r", a->r, 16) || !pointer("p", a->p, 16) || !pointer("x", a->x, 16)) return 1;
    } else {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 2) return refuse("which is not 0, 1 or 2"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (!pointer("partials", a->partials, 8)) return 1;
        if (a->hist_cap > 0 && !pointer("hist", a->hist, 8)) return 1;
    }

    PcgScalars h{};
    if (scalars != nullptr) memcpy(&h, scalars, sizeof h);
    PcgScalars* d_s = device_alloc<PcgScalars>(1);
    upload(d_s, &h, 1);
    double* stage_buf = nullptr;
    if (st == kInit) {
        launch_pcg_init(jac, a->n, a->b, a->Ap, a->dinv, a->r, a->p, a->partials);
        a->count = (int)stream_grid(a->n);
    } else if (st == kUpdateR) {
        launch_pcg_update_r(jac, a->n, d_s, a->Ap, a->dinv, a->r, a->partials);
        a->count = (int)stream_grid(a->n);
    } else if (st == kUpdateXp) {
        launch_pcg_update_xp(jac, a->n, d_s, a->r, a->dinv, a->p, a->x);
    } else {
        stage_buf = reduce_scratch_alloc();
        launch_pcg_reduce(a->partials, a->count, a->which == 1 ? 1 : 2, a->which, stage_buf, d_s, a->tol, a->hist, a->hist_cap);
    }
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
