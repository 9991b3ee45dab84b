// gcr.hip -- restarted GCR(m) (generalised conjugate residuals; mathematically FGMRES) over any SpmvOperator: the nonsymmetric loop
// that takes EVERY kind of SpmvAmdPrecond. It is flexible -- the preconditioner may change from iteration to
// iteration, so a polynomial or a V-cycle is as good as a matrix --, minimises the residual over the basis, so the recorded norm never
// grows, and under right preconditioning the recorded residual is the true one. Contract, statistics, timer rule, verbose semantics
// and stopping rule are spmv_amd_pcg_solve_device's (solve_common.hpp).
//
// The algebra (every fma is explicit, every other operation rounds once, the file is compiled with -ffp-contract=off); m = restart:
//   r = fma(1.0, b, -1.0 * (A x0)) ; ||r0|| = sqrt(r.r) ; history[0] = ||r0||
//   iteration k, slot j = k mod m (j == 0 empties the basis):
//   1. z = M^-1 r      "none": z is r ; "jacobi": dinv * r ; "chebyshev": section 14's application ; "multigrid": one V-cycle
//   2. q = A z         (the operator's own bits)
//   3. beta_i = (q.Q_i) / gamma_i, i = 0 .. j-1, ALL from the q of step 2 (classical Gram-Schmidt: one pass over the basis)
//   4. for i ascending: q = fma(-beta_i, Q_i, q) ; z = fma(-beta_i, Z_i, z)
//   5. gamma = q.q ; rho = r.q ; gamma or rho zero or not finite: BREAKDOWN -- the iteration counted, the unchanged residual recorded,
//      x untouched, converged = 0
//   6. alpha = rho / gamma ; x = fma(alpha, z, x) ; r = fma(-alpha, q, r) ; ||r|| = sqrt(r.r) recorded, the iteration counted, then the
//      strict stopping test
//   7. Z_j = z ; Q_j = q ; gamma_j = gamma
//
// Launches per iteration (streaming kernels in bicgstab.hip's style: one-wave workgroups on stream_grid(n), one 16-byte pair per lane,
// the odd last element by lane 0 of workgroup 0 after its pair, the loads before the scalars, wave_sum; value v of workgroup g at
// partials[v * count + g]); each group of sums and its scalar step are ONE launch of gcr_reduce_kernel, pcg_reduce_kernel's geometry
// per value on reduce_device.hpp's helpers:
//   the application (kinds with one) | the product q = A z INTO slot Q_j | multidot: the partials of q.Q_i, i < j (not at j = 0) | sum,
//   the betas (not at j = 0) | orthogonalise: step 4, Z_j written out of place and Q_j in place, the partials of q.q and r.q | sum,
//   alpha or the breakdown | the x / r kernel: step 6 with the partials of r.r ("jacobi": dinv r for the next product) | sum, ||r||, the
//   verdict
// then ONE small blocking read of the scalar record. The application and the product lie BEHIND that read, so a verdict wastes no
// product here; every other kernel tests the record's `stop` and returns at once.
//
// The chunk of basis vectors a lane holds in flight: kDotChunk = 8 in the multidot (8 x 16 B loads + Q_j's pair + the sums: 62
// VGPRs, so a SIMD keeps 8 waves and a CU 32 waves x 8 KiB of loads in flight, well past the ~32 KiB per CU that streaming from
// HBM takes), kOrthChunk = 4 in the orthogonalise kernel (a Q_i and a Z_i pair per slot: the same 8 loads beside q, z and r; 72
// VGPRs, 7 waves). Neither kernel spills. Q_j's pair is loaded once per lane, the chunks walk the basis behind it; a dot's bits do
// not depend on the chunk it fell into.
// Bytes per interior row and iteration on stencil5-csr, kind "none", slot j: product 56, multidot 8 (j + 1), orthogonalise 24 at
// j = 0 (z is r: one load) and 32 + 16 j behind it, x / r 48: 128 at j = 0, 144 + 24 j behind it. Workspace: x, b, r, 2 m basis
// vectors, the partials; "jacobi": dinv r; "chebyshev": d, z and a third vector.
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

constexpr int kMaxRestart = 32;
constexpr int kDefaultRestart = 16;
constexpr int kDotChunk = 8;   // basis vectors whose pairs a lane of the multidot kernel holds in flight
constexpr int kOrthChunk = 4;  // basis slots (a Q_i and a Z_i pair each) a lane of the orthogonalise kernel holds in flight

// Device scalars of one solve.
struct GcrScalars {
    double gamma[kMaxRestart];  // q.q of the basis slots filled since the last restart
    double beta[kMaxRestart];   // this iteration's (q.Q_i) / gamma_i, i < slot
    double alpha, rho;          // this iteration's step length and r.q
    double b_norm;              // ||r0||
    double residual;            // the norm recorded last
    int iterations;
    int converged;
    int breakdown;  // 0, or which scalar stopped the solve: 1 gamma = q.q, 2 rho = r.q
    int stop;       // the verdict: set with converged or breakdown; kernels behind it return at once
};

// The basis of one solve: slot i's Q_i = A Z_i (orthogonal) and Z_i, a 16-byte aligned allocation each. Slots >= j are never read.
struct GcrBasis {
    double* q[kMaxRestart];
    double* z[kMaxRestart];
};

// ---- the streaming kernels ----

// r = fma(1.0, b, -1.0 * Ax) ; the partials of r.r ; "jacobi": zs = dinv r for the first product
template <bool kJac>
__global__ __launch_bounds__(kWave) void gcr_init_kernel(size_t n, const double* __restrict__ b, const double* __restrict__ Ax,
                                                         const double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ zs,
                                                         double* __restrict__ partials) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    double rr = 0.0;
    if (i < (n >> 1)) {
        const d2 bv = load_once(b, i), av = load_once(Ax, i);
        d2 rv;
        rv.x = fma(1.0, bv.x, -1.0 * av.x);
        rv.y = fma(1.0, bv.y, -1.0 * av.y);
        if (kJac) {
            const d2 dv = load_once(dinv, i);
            d2 hv;
            hv.x = dv.x * rv.x, hv.y = dv.y * rv.y;
            store_once(r, i, rv);
            reinterpret_cast<d2*>(zs)[i] = hv;  // plain: the first product reads it
        } else {
            reinterpret_cast<d2*>(r)[i] = rv;  // plain: the first application or product reads it
        }
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double rl = fma(1.0, b[n - 1], -1.0 * Ax[n - 1]);
        r[n - 1] = rl;
        if (kJac) zs[n - 1] = dinv[n - 1] * rl;
        rr = fma(rl, rl, rr);
    }
    rr = wave_sum(rr);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr;
}

// The partials of Q_i.q, i = 0 .. j-1 (value i at partials[i * count + g]), q = Q_j: one pass over the basis, q's pair loaded once.
__global__ __launch_bounds__(kWave) void gcr_multidot_kernel(size_t n, const GcrScalars* __restrict__ s, GcrBasis basis, int j,
                                                             double* __restrict__ partials, int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    const bool last = (n & 1) && blockIdx.x == 0 && threadIdx.x == 0;
    const double* const q = basis.q[j];
    d2 qv = {0.0, 0.0};
    if (live) qv = load_once(q, i);
    const double ql = last ? q[n - 1] : 0.0;
    for (int base = 0; base < j; base += kDotChunk) {
        d2 av[kDotChunk];
        double al[kDotChunk];
#pragma unroll
        for (int u = 0; u < kDotChunk; ++u) {  // the loads before the scalars
            const double* const a = basis.q[base + u < j ? base + u : j];
            av[u] = d2{0.0, 0.0}, al[u] = 0.0;
            if (live && base + u < j) av[u] = load_once(a, i);
            if (last && base + u < j) al[u] = a[n - 1];
        }
        if (s->stop != 0) return;
#pragma unroll
        for (int u = 0; u < kDotChunk; ++u) {
            if (base + u >= j) break;  // uniform
            double ab = 0.0;
            if (live) ab = fma(av[u].x, qv.x, ab), ab = fma(av[u].y, qv.y, ab);
            if (last) ab = fma(al[u], ql, ab);
            ab = wave_sum(ab);
            if (threadIdx.x == 0) partials[(size_t)(base + u) * count + blockIdx.x] = ab;
        }
    }
}

// Step 4 with i ascending on q = Q_j (in place) and z = z_in (out of place into Z_j), then the partials of q.q (value 0) and r.q
// (value 1). z_in: wherever the application left z -- r itself ("none": loaded once), the "jacobi" scratch, the Chebyshev z, the
// cycle's vector. At j = 0 z moves into Z_0 and q stays where the product wrote it.
__global__ __launch_bounds__(kWave) void gcr_orthogonalise_kernel(size_t n, const GcrScalars* __restrict__ s, const double* z_in,
                                                                  GcrBasis basis, int j, const double* r, double* __restrict__ partials,
                                                                  int count) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    const bool last = (n & 1) && blockIdx.x == 0 && threadIdx.x == 0;
    const bool z_is_r = z_in == r;
    double* const q = basis.q[j];
    double* const z = basis.z[j];
    d2 qv = {0.0, 0.0}, zv = {0.0, 0.0}, rv = {0.0, 0.0};
    double ql = 0.0, zl = 0.0, rl = 0.0;
    if (live) {  // the loads before the scalars
        qv = load_once(q, i);
        zv = load_once(z_in, i);
        rv = z_is_r ? zv : load_once(r, i);
    }
    if (last) ql = q[n - 1], zl = z_in[n - 1], rl = r[n - 1];
    if (j == 0 && s->stop != 0) return;
    for (int base = 0; base < j; base += kOrthChunk) {
        d2 av[kOrthChunk], cv[kOrthChunk];
        double al[kOrthChunk], cl[kOrthChunk];
#pragma unroll
        for (int u = 0; u < kOrthChunk; ++u) {
            const int slot = base + u < j ? base + u : 0;
            av[u] = cv[u] = d2{0.0, 0.0}, al[u] = cl[u] = 0.0;
            if (live && base + u < j) av[u] = load_once(basis.q[slot], i), cv[u] = load_once(basis.z[slot], i);
            if (last && base + u < j) al[u] = basis.q[slot][n - 1], cl[u] = basis.z[slot][n - 1];
        }
        if (s->stop != 0) return;
#pragma unroll
        for (int u = 0; u < kOrthChunk; ++u) {
            if (base + u >= j) break;  // uniform
            const double nb = -s->beta[base + u];
            qv.x = fma(nb, av[u].x, qv.x), qv.y = fma(nb, av[u].y, qv.y);
            zv.x = fma(nb, cv[u].x, zv.x), zv.y = fma(nb, cv[u].y, zv.y);
            ql = fma(nb, al[u], ql), zl = fma(nb, cl[u], zl);
        }
    }
    double qq = 0.0, rq = 0.0;
    if (live) {
        if (j > 0) store_once(q, i, qv);
        store_once(z, i, zv);
        qq = fma(qv.x, qv.x, qq), qq = fma(qv.y, qv.y, qq);
        rq = fma(rv.x, qv.x, rq), rq = fma(rv.y, qv.y, rq);
    }
    if (last) {
        if (j > 0) q[n - 1] = ql;
        z[n - 1] = zl;
        qq = fma(ql, ql, qq), rq = fma(rl, ql, rq);
    }
    qq = wave_sum(qq), rq = wave_sum(rq);
    if (threadIdx.x == 0) partials[blockIdx.x] = qq, partials[count + blockIdx.x] = rq;
}

// x = fma(alpha, z, x) ; r = fma(-alpha, q, r) ; the partials of r.r ; "jacobi": zs = dinv r for the next product. z = Z_j, q = Q_j.
template <bool kJac>
__global__ __launch_bounds__(kWave) void gcr_update_xr_kernel(size_t n, const GcrScalars* __restrict__ s, const double* __restrict__ z,
                                                              const double* __restrict__ q, const double* __restrict__ dinv,
                                                              double* __restrict__ x, double* __restrict__ r, double* __restrict__ zs,
                                                              double* __restrict__ partials) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    const bool live = i < (n >> 1);
    d2 xv = {0.0, 0.0}, zv = {0.0, 0.0}, rv = {0.0, 0.0}, qv = {0.0, 0.0}, dv = {1.0, 1.0};
    if (live) {  // the loads before the scalars
        xv = load_once(x, i);
        zv = load_once(z, i);
        rv = load_once(r, i);
        qv = load_once(q, i);
        if (kJac) dv = load_once(dinv, i);
    }
    if (s->stop != 0) return;
    const double alpha = s->alpha;
    double rr = 0.0;
    if (live) {
        xv.x = fma(alpha, zv.x, xv.x), xv.y = fma(alpha, zv.y, xv.y);
        rv.x = fma(-alpha, qv.x, rv.x), rv.y = fma(-alpha, qv.y, rv.y);
        store_once(x, i, xv);
        if (kJac) {
            d2 hv;
            hv.x = dv.x * rv.x, hv.y = dv.y * rv.y;
            store_once(r, i, rv);
            reinterpret_cast<d2*>(zs)[i] = hv;  // plain: the next product reads it
        } else {
            reinterpret_cast<d2*>(r)[i] = rv;  // plain: the next application or product reads it
        }
        rr = fma(rv.x, rv.x, rr), rr = fma(rv.y, rv.y, rr);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        x[n - 1] = fma(alpha, z[n - 1], x[n - 1]);
        const double rl = fma(-alpha, q[n - 1], r[n - 1]);
        r[n - 1] = rl;
        if (kJac) zs[n - 1] = dinv[n - 1] * rl;
        rr = fma(rl, rl, rr);
    }
    rr = wave_sum(rr);
    if (threadIdx.x == 0) partials[blockIdx.x] = rr;
}

// ---- reductions: nv (1 .. 31) sums of `count` partials each (value v at partials[v * count ...]) in ONE launch, then the scalar
// step. pcg_reduce_kernel's geometry per value: one workgroup up to 1024 partials, else slice workgroups that publish their slice sum
// of value v into slices[v * kReduceStageBlocks + slot]; the workgroup that draws the last ticket sums them and takes the step.
// which: 0 = r0.r0 ; 1 = the betas of slot j (nv = j) ; 2 = gamma and rho (nv = 2): alpha or the breakdown ; 3 = r.r: ||r|| and the
// verdict. Steps 1 to 3 lie behind a verdict: every workgroup reads `stop` before it draws a ticket, and the step writes it only
// after the last ticket is drawn. ----

__device__ __forceinline__ void gcr_record(GcrScalars* s, double norm, double* hist, int hist_cap) {
    s->iterations += 1;
    s->residual = norm;
    if (s->iterations < hist_cap) hist[s->iterations] = norm;
}

__device__ void gcr_step(GcrScalars* s, int which, int j, const double* total, double tol, double* hist, int hist_cap) {
    if (which == 0) {
        for (int i = 0; i < kMaxRestart; ++i) s->gamma[i] = s->beta[i] = 0.0;
        s->alpha = s->rho = 0.0;
        s->b_norm = sqrt(total[0]);
        s->residual = s->b_norm;
        s->iterations = s->converged = s->breakdown = s->stop = 0;
        if (hist_cap > 0) hist[0] = s->b_norm;
    } else if (which == 1) {
        for (int i = 0; i < j; ++i) s->beta[i] = total[i] / s->gamma[i];
    } else if (which == 2) {
        s->rho = total[1];
        if (usable(total[0]) && usable(total[1])) {
            s->gamma[j] = total[0];
            s->alpha = total[1] / total[0];
        } else {
            s->alpha = 0.0;
            s->breakdown = usable(total[0]) ? 2 : 1, s->stop = 1;
            gcr_record(s, s->residual, hist, hist_cap);
        }
    } else {
        const double res = sqrt(total[0]);
        gcr_record(s, res, hist, hist_cap);
        if (res / s->b_norm < tol) s->converged = 1, s->stop = 1;
    }
}

__global__ __launch_bounds__(kReduceBlock) void gcr_reduce_kernel(const double* __restrict__ partials, int count, int nv, int slice, int blocks,
                                                                  double* stage_base, unsigned long long* slices, GcrScalars* s, int which,
                                                                  int j, double tol, double* hist, int hist_cap) {
    __shared__ double sh[kReduceBlock];
    __shared__ double total[kMaxRestart];
    __shared__ int s_last;
    if (which >= 1 && s->stop != 0) return;
    const auto slot_of = [&](int v) { return slices + (size_t)v * kReduceStageBlocks; };
    if (!sum_values_last_block<0>(partials, count, nv, slice, blocks, reduce_stage_of(stage_base).ticket, slot_of, sh, &s_last, total)) return;
    if (threadIdx.x == 0) gcr_step(s, which, j, total, tol, hist, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_gcr_stage ----

// What the launches of one solve (or one stage call) work on.
struct GcrVectors {
    bool jac = false;
    size_t n = 0;
    const double* b = nullptr;
    const double* Ax = nullptr;    // init: A x0
    const double* dinv = nullptr;  // "jacobi"
    double *x = nullptr, *r = nullptr;
    double* zs = nullptr;          // "jacobi": dinv r
    const double* z_in = nullptr;  // orthogonalise: where the application left z
    GcrBasis basis{};
    double* partials = nullptr;
    GcrScalars* s = nullptr;
};

#define GCR_LAUNCH(kernel, ...) SPMV_AMD_STREAM_LAUNCH(kernel, a.jac, a.n, __VA_ARGS__)
void launch_gcr_init(const GcrVectors& a) { GCR_LAUNCH(gcr_init_kernel, a.b, a.Ax, a.dinv, a.r, a.zs, a.partials); }
void launch_gcr_update_xr(const GcrVectors& a, int j) {
    GCR_LAUNCH(gcr_update_xr_kernel, a.s, a.basis.z[j], a.basis.q[j], a.dinv, a.x, a.r, a.zs, a.partials);
}
#undef GCR_LAUNCH

void launch_gcr_multidot(const GcrVectors& a, int j) {
    const dim3 grid(stream_grid(a.n)), block(kWave);
    hipLaunchKernelGGL(gcr_multidot_kernel, grid, block, 0, kStream, a.n, a.s, a.basis, j, a.partials, (int)grid.x);
}
void launch_gcr_orthogonalise(const GcrVectors& a, int j) {
    const dim3 grid(stream_grid(a.n)), block(kWave);
    hipLaunchKernelGGL(gcr_orthogonalise_kernel, grid, block, 0, kStream, a.n, a.s, a.z_in, a.basis, j, a.r, a.partials, (int)grid.x);
}

// the sums of `count` partials per value and the scalar step `which` of slot j (0, 3: one value; 1: j values; 2: two)
void launch_gcr_reduce(const double* partials, int count, int which, int j, double* stage, unsigned long long* slices, GcrScalars* s,
                       double tol, double* hist, int hist_cap) {
    int slice = 0, blocks = 0;
    reduce_geometry(count, &slice, &blocks);
    const int nv = which == 1 ? j : which == 2 ? 2 : 1;
    hipLaunchKernelGGL(gcr_reduce_kernel, dim3((unsigned)blocks), dim3(kReduceBlock), 0, kStream, partials, count, nv, slice, blocks, stage,
                       slices, s, which, j, tol, hist, hist_cap);
}

// ---- workspace: kept between calls, released with the other CG workspaces ----
constexpr size_t kSliceSlots = (size_t)kMaxRestart * kReduceStageBlocks;

// What a kind adds to x, b, r and the basis: "jacobi" dinv r; "chebyshev" d, z and the third vector of a step.
int scratch_vectors(int kind) { return kind == kJacobi ? 1 : kind == kChebyshev ? 3 : 0; }
// The partials are kMaxRestart values wide whatever the restart: a workspace serves every restart, and a unit of restart costs its
// two basis vectors and nothing else.
size_t partial_slots(int n) { return (size_t)kMaxRestart * stream_grid((size_t)n); }
size_t workspace_bytes_of(int n, int restart, int kind) {
    return ((size_t)(3 + 2 * restart + scratch_vectors(kind)) * (size_t)n + partial_slots(n)) * sizeof(double);
}

struct GcrWorkspace {
    int n = 0, device = -1, slots = 0;
    double *x = nullptr, *b = nullptr, *r = nullptr;
    GcrBasis basis{};
    double* zs = nullptr;                                  // kind "jacobi" only
    double *cd = nullptr, *cz = nullptr, *cz2 = nullptr;   // kind "chebyshev" only: d, z and the fused step's second z (else A z)
    double* cpartials = nullptr;                           // and the slots its step launches write
    long long cpartial_cap = 0;
    double* partials = nullptr;  // kMaxRestart x streaming workgroups
    double* stage = nullptr;     // reduce_scratch_alloc(): the ticket
    unsigned long long* slices = nullptr;
    GcrScalars* s = nullptr;
    double* hist = nullptr;
    int hist_cap = 0;
    void release() {
        for (int i = 0; i < kMaxRestart; ++i) {
            device_release(basis.q[i]);
            device_release(basis.z[i]);
        }
        device_release(zs);
        device_release(cd);
        device_release(cz);
        device_release(cz2);
        device_release(cpartials);
        device_release(x);
        device_release(b);
        device_release(r);
        device_release(partials);
        device_release(stage);
        device_release(slices);
        device_release(s);
        device_release(hist);
        n = 0, device = -1, slots = 0, hist_cap = 0, cpartial_cap = 0;
    }
};
GcrWorkspace g_gcr;
std::vector<double> g_gcr_history;  // of the last solve

bool fail(const char* what) {
    fprintf(stderr, "[GCR] %s\n", what);
    return false;
}

// Sized against free memory before anything is allocated. need: what this request adds; fixed: the part of it that does not grow with
// the restart; held: basis slots the workspace has already. A request that does not fit names the largest restart that would.
bool has_room(size_t need, size_t fixed, int n, int restart, int held) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need <= free_b) return true;
    const size_t per_unit = 2 * (size_t)n * sizeof(double);
    long long fits = held + (free_b > fixed ? (long long)((free_b - fixed) / per_unit) : 0);
    if (fits >= restart) fits = restart - 1;
    char largest[64];
    if (fits >= 1) snprintf(largest, sizeof largest, "restart %lld is the largest that fits", fits);
    else snprintf(largest, sizeof largest, "no restart fits");
    fprintf(stderr, "[GCR] the workspace for %d rows at restart %d needs %.2f GB more, the device has %.2f GB free: refused (%s)\n", n, restart,
            need / 1e9, free_b / 1e9, largest);
    return false;
}

bool ensure_workspace(int n, int device, int restart, int kind, long long cheb_partials, int hist_cap) {
    GcrWorkspace& w = g_gcr;
    if (w.x != nullptr && (w.n != n || w.device != device)) w.release();
    const size_t vec = (size_t)n * sizeof(double), margin = (size_t)64 << 20;
    if (w.x == nullptr) {
        const size_t fixed = workspace_bytes_of(n, 0, kind) + (size_t)hist_cap * sizeof(double) + margin;
        if (!has_room(fixed + 2 * (size_t)restart * vec, fixed, n, restart, 0)) return false;
        w.x = device_try_alloc<double>((size_t)n);
        w.b = device_try_alloc<double>((size_t)n);
        w.r = device_try_alloc<double>((size_t)n);
        w.partials = device_try_alloc<double>(partial_slots(n));
        w.slices = device_try_alloc<unsigned long long>(kSliceSlots);
        w.s = device_try_alloc<GcrScalars>(1);
        if (!w.x || !w.b || !w.r || !w.partials || !w.slices || !w.s) {
            w.release();
            return fail("the workspace could not be allocated: refused");
        }
        w.stage = reduce_scratch_alloc();
        w.n = n, w.device = device;
    } else if (restart > w.slots) {
        if (!has_room(2 * (size_t)(restart - w.slots) * vec + margin, margin, n, restart, w.slots)) return false;
    }
    for (; w.slots < restart; ++w.slots) {
        w.basis.q[w.slots] = device_try_alloc<double>((size_t)n);
        w.basis.z[w.slots] = device_try_alloc<double>((size_t)n);
        if (!w.basis.q[w.slots] || !w.basis.z[w.slots]) {
            w.release();
            return fail("the basis vectors could not be allocated: refused");
        }
    }
    if (kind == kJacobi && w.zs == nullptr) {
        if (!has_room(vec + margin, vec + margin, n, restart, restart)) return false;
        w.zs = device_try_alloc<double>((size_t)n);
        if (!w.zs) return fail("the Jacobi vector could not be allocated: refused");
    }
    if (kind == kChebyshev) {
        if (w.cd == nullptr) {
            if (!has_room(3 * vec + margin, 3 * vec + margin, n, restart, restart)) return false;
            w.cd = device_try_alloc<double>((size_t)n);
            w.cz = device_try_alloc<double>((size_t)n);
            w.cz2 = device_try_alloc<double>((size_t)n);
            if (!w.cd || !w.cz || !w.cz2) {
                device_release(w.cd);
                device_release(w.cz);
                device_release(w.cz2);
                return fail("the Chebyshev vectors could not be allocated: refused");
            }
        }
        if (w.cpartial_cap < cheb_partials) {
            device_release(w.cpartials);
            w.cpartial_cap = 0;
            w.cpartials = device_try_alloc<double>((size_t)cheb_partials);
            if (!w.cpartials) return fail("the Chebyshev partials could not be allocated: refused");
            w.cpartial_cap = cheb_partials;
        }
    }
    if (!grow_history(w.hist, w.hist_cap, hist_cap)) return fail("the history could not be allocated: refused");
    return true;
}

}  // namespace

namespace spmv_amd {
void release_gcr_workspace_locked() { g_gcr.release(); }
}  // namespace spmv_amd

extern "C" size_t spmv_amd_gcr_workspace_bytes(int rows, int restart, const char* kind) {
    const int k = kind_of(kind);
    if (rows < 1 || restart < 0 || restart > kMaxRestart || k < 0) return 0;
    return workspace_bytes_of(rows, restart == 0 ? kDefaultRestart : restart, k);
}

extern "C" int spmv_amd_gcr_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int restart, const double* b, double* x,
                                         const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (!check_solve_arguments("GCR", op, mat, m, b, x, config, stats)) return 1;
    if (restart < 0 || restart > kMaxRestart) {
        fprintf(stderr, "[GCR] restart = %d: 1 .. %d, or 0 for the default %d: refused\n", restart, kMaxRestart, kDefaultRestart);
        return 1;
    }
    if (m->kind != kNone && m->kind != kJacobi && m->kind != kChebyshev && m->kind != kMultigrid)
        return fail("the preconditioner record is not one of this library's (unknown kind): refused"), 1;
    if (!check_solve_system("GCR", op, mat, m)) return 1;
    const int n = mat->rows;
    const int mr = restart == 0 ? kDefaultRestart : restart;
    const CGConfig cfg = *config;
    const bool jac = m->kind == kJacobi, cheb = m->kind == kChebyshev, mg = m->kind == kMultigrid;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const int count = (int)stream_grid((size_t)n);
    const ChebSpmv spmv = cheb ? cheb_spmv_of(op) : ChebSpmv{};
    const long long cheb_partials = spmv.partials > count ? (long long)spmv.partials : (long long)count;
    if (!ensure_workspace(n, device, mr, m->kind, cheb_partials, cfg.max_iters + 1)) return 1;
    GcrWorkspace& w = g_gcr;
    upload(w.b, b, (size_t)n);
    upload(w.x, x, (size_t)n);

    GcrVectors a;
    a.jac = jac, a.n = (size_t)n, a.b = w.b, a.Ax = w.basis.q[0], a.dinv = jac ? m->dinv : nullptr, a.x = w.x, a.r = w.r;
    a.zs = jac ? w.zs : nullptr, a.basis = w.basis, a.partials = w.partials, a.s = w.s;
    StageTimers T(cfg.enable_detailed_timers != 0, kStream);
    bool failed = false;
    auto product = [&](const double* in, double* out) { timed_product("GCR", op, T, in, out, failed); };
    auto reduce = [&](int which, int j) {
        T.run(&T.t_red, [&] { launch_gcr_reduce(w.partials, count, which, j, w.stage, w.slices, w.s, cfg.tolerance, w.hist, w.hist_cap); });
    };
    // step 1: where z = M^-1 r is once the application's launches are enqueued (null: run_device refused)
    auto apply = [&]() -> const double* {
        if (jac) return w.zs;
        if (mg) return mg_cycle(m->mg, w.r, &T).z;
        if (!cheb) return w.r;
        ChebRun c;
        c.a = spmv, c.n = (size_t)n, c.r = w.r, c.dinv = m->dinv, c.d = w.cd, c.z = w.cz, c.aux = w.cz2, c.partials = w.cpartials, c.T = &T;
        T.run(&T.t_blas, [&] { launch_cheb_term0_apply((size_t)n, w.r, m->dinv, m->coef[0], w.cd, w.cz); });
        if (!cheb_steps(c, m->degree, m->coef, false)) return failed = true, nullptr;
        return c.z;
    };
    GcrScalars h{};

    T.total.begin(kStream);
    product(w.x, w.basis.q[0]);  // A x0 into slot 0, which the first product of the loop overwrites
    if (!failed) {
        T.run(&T.t_blas, [&] { launch_gcr_init(a); });
        reduce(0, 0);
        download(&h, w.s, 1);
        if (cfg.verbose >= 1) printf("[GCR-DEVICE] Initial residual: %e (preconditioner %s, restart %d)\n", h.b_norm, spmv_amd_precond_kind(m), mr);
    }
    for (int it = 0; it < cfg.max_iters && !failed && !h.converged && !h.breakdown; ++it) {
        const int j = it % mr;
        a.z_in = apply();
        if (failed || a.z_in == nullptr) break;
        product(a.z_in, w.basis.q[j]);  // q = A z into slot j
        if (failed) break;
        if (j > 0) {
            T.run(&T.t_blas, [&] { launch_gcr_multidot(a, j); });
            reduce(1, j);  // the betas
        }
        T.run(&T.t_blas, [&] { launch_gcr_orthogonalise(a, j); });
        reduce(2, j);  // gamma, rho, alpha -- or the breakdown
        T.run(&T.t_blas, [&] { launch_gcr_update_xr(a, j); });
        reduce(3, j);  // ||r|| and the verdict
        download(&h, w.s, 1);  // synchronises: the one blocking read of the iteration
        if (cfg.verbose >= 2) printf("[GCR-DEVICE] Iter %3d: residual = %e (rel = %e)\n", h.iterations, h.residual, h.residual / h.b_norm);
    }
    T.total.end(kStream);
    const double total_ms = T.total.elapsed_ms();
    HIP_CHECK(hipGetLastError());
    if (failed) {
        HIP_CHECK(hipDeviceSynchronize());
        return 1;
    }
    download_solution(x, w.x, n, h.iterations, w.hist, w.hist_cap, g_gcr_history);

    static const char* const scalar[] = {"", "gamma = q.q", "rho = r.q", ""};
    const SolveSummary done{h.iterations, h.converged != 0, h.residual, h.b_norm, h.breakdown ? scalar[h.breakdown & 3] : nullptr};
    report_solve("GCR", done, x, n, cfg, T, total_ms, stats);
    return 0;
}

extern "C" int spmv_amd_gcr_last_history(double* out, int cap) { return copy_history(g_gcr_history, out, cap); }

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_gcr_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdGcrScalars) == sizeof(GcrScalars) && offsetof(SpmvAmdGcrScalars, beta) == offsetof(GcrScalars, beta) &&
                  offsetof(SpmvAmdGcrScalars, alpha) == offsetof(GcrScalars, alpha) && offsetof(SpmvAmdGcrScalars, rho) == offsetof(GcrScalars, rho) &&
                  offsetof(SpmvAmdGcrScalars, b_norm) == offsetof(GcrScalars, b_norm) &&
                  offsetof(SpmvAmdGcrScalars, residual) == offsetof(GcrScalars, residual) &&
                  offsetof(SpmvAmdGcrScalars, iterations) == offsetof(GcrScalars, iterations) &&
                  offsetof(SpmvAmdGcrScalars, breakdown) == offsetof(GcrScalars, breakdown) &&
                  offsetof(SpmvAmdGcrScalars, stop) == offsetof(GcrScalars, stop),
              "lab.h's scalar record is the device record, field for field");
static_assert(SPMV_AMD_GCR_MAX_RESTART == kMaxRestart && SPMV_AMD_GCR_DOT_CHUNK == kDotChunk && SPMV_AMD_GCR_ORTH_CHUNK == kOrthChunk,
              "lab.h states the solver's restart limit and chunk sizes");

extern "C" int spmv_amd_gcr_stage(const char* stage, const char* kind, SpmvAmdGcrStageArgs* a, SpmvAmdGcrScalars* scalars) {
    // argument checks: all before the first HIP call. 16: a vector the streaming kernels read or write in 16-byte pairs; 8: an array
    // of doubles read or written one at a time
    static const char* const kStages = "init, multidot, orthogonalise, update_xr, reduce";
    char names[96];
    auto refuse = [&](const char* what) { return stage_fail("GCR", stage, what); };
    auto pointer = [&](const char* name, const void* ptr) { return stage_pointer("GCR", stage, name, ptr, 16); };
    enum { kInit, kMultidot, kOrth, kUpdateXr, kReduce } st;
    if (stage == nullptr) {
        snprintf(names, sizeof names, "no stage named (%s)", kStages);
        return refuse(names), 1;
    }
    if (!strcmp(stage, "init")) st = kInit;
    else if (!strcmp(stage, "multidot")) st = kMultidot;
    else if (!strcmp(stage, "orthogonalise")) st = kOrth;
    else if (!strcmp(stage, "update_xr")) st = kUpdateXr;
    else if (!strcmp(stage, "reduce")) st = kReduce;
    else {
        snprintf(names, sizeof names, "unknown stage (%s)", kStages);
        return refuse(names), 1;
    }
    if (a == nullptr) return refuse("null arguments"), 1;
    bool jac = false;
    if (st == kInit || st == kUpdateXr) {
        const int k = kind_of(kind);
        if (k != kNone && k != kJacobi) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
        jac = k == kJacobi;
    }
    if (st != kReduce && (a->n < 1 || a->n > (size_t)INT_MAX)) return refuse("n < 1 or beyond the solver's int rows"), 1;
    if (st != kInit && scalars == nullptr) return refuse("null scalar record"), 1;
    if (st != kInit) {
        const int lo = st == kMultidot ? 1 : 0;
        if (a->slot < lo || a->slot >= kMaxRestart) return refuse(st == kMultidot ? "slot outside 1 .. 31" : "slot outside 0 .. 31"), 1;
    }
    if (jac && !pointer("dinv", a->dinv)) return 1;
    if (jac && !pointer("zs", a->zs)) return 1;
    GcrBasis basis{};
    if (st == kInit) {
        if (!pointer("b", a->b) || !pointer("v", a->v) || !pointer("r", a->r)) return 1;
    } else if (st != kReduce) {
        if (a->Q == nullptr) return refuse("Q is null"), 1;
        if (st != kMultidot && a->Z == nullptr) return refuse("Z is null"), 1;
        const int j = a->slot;
        char name[16];
        for (int i = st == kUpdateXr ? j : 0; i <= j; ++i) {  // slots > j are not looked at
            snprintf(name, sizeof name, "Q[%d]", i);
            if (!pointer(name, a->Q[i])) return 1;
            basis.q[i] = a->Q[i];
            if (st == kMultidot) continue;
            snprintf(name, sizeof name, "Z[%d]", i);
            if (!pointer(name, a->Z[i])) return 1;
            basis.z[i] = a->Z[i];
        }
        if (st == kOrth && (!pointer("z_in", a->z_in) || !pointer("r", a->r))) return 1;
        if (st == kUpdateXr && (!pointer("x", a->x) || !pointer("r", a->r))) return 1;
    } else {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 3) return refuse("which is not 0, 1, 2 or 3"), 1;
        if (a->which == 1 && a->slot < 1) return refuse("slot outside 1 .. 31"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (a->hist_cap > 0 && !stage_pointer("GCR", stage, "hist", a->hist, 8)) return 1;
    }
    if (!stage_pointer("GCR", stage, "partials", a->partials, 8)) return 1;

    GcrScalars h{};
    if (scalars != nullptr) memcpy(&h, scalars, sizeof h);
    GcrScalars* d_s = device_alloc<GcrScalars>(1);
    upload(d_s, &h, 1);
    GcrVectors w;
    w.jac = jac, w.n = a->n, w.b = a->b, w.Ax = a->v, w.dinv = a->dinv, w.x = a->x, w.r = a->r, w.zs = a->zs, w.z_in = a->z_in;
    w.basis = basis, w.partials = a->partials, w.s = d_s;
    double* stage_buf = nullptr;
    unsigned long long* slices = nullptr;
    if (st == kInit) launch_gcr_init(w);
    else if (st == kMultidot) launch_gcr_multidot(w, a->slot);
    else if (st == kOrth) launch_gcr_orthogonalise(w, a->slot);
    else if (st == kUpdateXr) launch_gcr_update_xr(w, a->slot);
    else {
        stage_buf = reduce_scratch_alloc();
        slices = device_alloc<unsigned long long>(kSliceSlots);
        launch_gcr_reduce(a->partials, a->count, a->which, a->slot, stage_buf, slices, d_s, a->tol, a->hist, a->hist_cap);
    }
    if (st != kReduce) a->count = (int)stream_grid(a->n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (st == kReduce) {
        download(&h, d_s, 1);
        memcpy(scalars, &h, sizeof h);
    }
    device_release(stage_buf);
    device_release(slices);
    device_release(d_s);
    return 0;
}
#endif  // SPMV_AMD_LAB
