// pcg.hip -- preconditioned CG over any SpmvOperator: kinds "none" and "jacobi" (DESIGN.md section 13), a Chebyshev polynomial in
// D^-1 A (section 14) and one multigrid V-cycle (multigrid.hip, section 15: stencil5-csr; section 17: stencil7-csr). The solver only:
// the preconditioner record, its creators and its application on its own are precond.hip's; the host side this loop shares with
// bicgstab.hip and gcr.hip is single_solve.hpp's.
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
// A step is cheb_step (precond.hip, declared in precond.hpp), the only place that chooses its form from a ChebSpmv: on a row-lds stencil plan ONE
// launch (spmv_kernels.hip, kMode 3: A z never leaves the registers, z' goes to a second vector; 144 + 88 k bytes per interior row and
// iteration), on any other stencil plan -- 2-D, or a 3-D multigrid level's Stencil7Plan -- the SpMV behind the flag +
// cheb_step_kernel, else run_device + cheb_step_kernel (112 per step). The loop calls it timed, with the flag and the step counter; spmv_amd_precond_apply_device untimed without a flag; the
// multigrid cycle on each of its levels.
//
// "multigrid" (mg_first, mg_next): z = M^-1 r is one V-cycle on the preconditioner's own levels:
//   r -= alpha Ap with the r.r partials (the "none" r update) | sum of r.r + verdict | the host reads the verdict: the converging
//   iteration runs no cycle | V-cycle | sum of r.z + beta
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

// ---- kind "chebyshev": term 0 fused into the r update ----

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
    const ReduceStage stage = reduce_stage_of(stage_base);
    const auto slot_of = [&](int v) { return v == 0 ? stage.sums : stage.extra; };
    if (!sum_values_last_block<NV>(partials, count, NV, slice, blocks, stage.ticket, slot_of, sh, &s_last, total)) return;
    if (threadIdx.x == 0) pcg_step(s, which, total, tol, hist, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_pcg_stage (the
// kernels on caller data, tests/test_pcg_stages_gpu.py). dinv is not read by the "none" instantiations. ----

void launch_pcg_init(bool jac, size_t n, const double* b, const double* Ap, const double* dinv, double* r, double* p, double* partials) {
    SPMV_AMD_STREAM_LAUNCH(pcg_init_kernel, jac, n, b, Ap, dinv, r, p, partials, count);
}
void launch_pcg_update_r(bool jac, size_t n, const PcgScalars* s, const double* Ap, const double* dinv, double* r, double* partials) {
    SPMV_AMD_STREAM_LAUNCH(pcg_update_r_kernel, jac, n, s, Ap, dinv, r, partials, count);
}
void launch_pcg_update_xp(bool jac, size_t n, const PcgScalars* s, const double* r, const double* dinv, double* p, double* x) {
    SPMV_AMD_STREAM_LAUNCH(pcg_update_xp_kernel, jac, n, s, r, dinv, p, x);
}

}  // namespace

// nv sums of `count` partials each and the scalar step `which` (0: two sums, 1: one, 2: two)
void spmv_amd::launch_pcg_reduce(const double* partials, int count, int nv, int which, double* stage, PcgScalars* s, double tol,
                                 double* hist, int hist_cap) {
    int slice = 0, blocks = 0;
    reduce_geometry(count, &slice, &blocks);
    if (nv == 1)
        hipLaunchKernelGGL(pcg_reduce_kernel<1>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
    else
        hipLaunchKernelGGL(pcg_reduce_kernel<2>, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, slice, blocks, stage,
                           s, which, tol, hist, hist_cap);
}

namespace {

// ---- kind "chebyshev": the launches ----

template <int kFrom>
void launch_cheb_term0(size_t n, const PcgScalars* s, const double* b, const double* Ap, const double* dinv, double c0, double* r, double* d,
                       double* z, bool last, double* partials) {
    const dim3 grid(stream_grid(n)), block(kWave);
    hipLaunchKernelGGL(cheb_term0_kernel<kFrom>, grid, block, 0, kStream, n, s, b, Ap, dinv, c0, r, d, z, last ? 1 : 0, partials, (int)grid.x);
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

}  // namespace

namespace spmv_amd {
void release_pcg_workspace_locked() { g_pcg.release(); }
}  // namespace spmv_amd

// term 0 for an application on its own (precond.hpp: precond.hip, gcr.hip)
void spmv_amd::launch_cheb_term0_apply(size_t n, const double* r, const double* dinv, double c0, double* d, double* z, bool last,
                                       double* partials) {
    launch_cheb_term0<2>(n, nullptr, nullptr, nullptr, dinv, c0, const_cast<double*>(r), d, z, last, partials);
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
    void product(const double* in, double* out) { timed_product("PCG", op, T, in, out, failed); }  // out = A in through the vtable
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
    L.product(w.x, w.Ap);
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
    L.product(w.x, w.Ap);
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
    L.product(w.x, w.Ap);
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
    if (!check_solve_arguments("PCG", op, mat, m, b, x, config, stats) || !check_solve_system("PCG", op, mat, m)) return 1;
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
                operator_product("PCG", op, w.p, w.Ap, L.failed);
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
    download_solution(x, w.x, n, h.iterations, w.hist, w.hist_cap, g_pcg_history);
    g_mg_cycles = L.cycles;
    g_cheb_step_launches = 0;
    if (L.step_counter != nullptr) download(&g_cheb_step_launches, L.step_counter, 1);
    if (L.failed) return 1;

    const SolveSummary done{h.iterations, h.converged != 0, h.residual, h.b_norm, h.breakdown ? "pAp or r.z" : nullptr};
    report_solve("PCG", done, x, n, cfg, T, total_ms, stats);
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
        if (k != kNone && k != kJacobi) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
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
