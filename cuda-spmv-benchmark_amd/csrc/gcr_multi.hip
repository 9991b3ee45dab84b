// gcr_multi.hip -- batched GCR(m): up to 8 independent nonsymmetric systems A x_j = b_j solved together under one preconditioner of
// ANY kind ("none", "jacobi", "chebyshev", "multigrid" on a hierarchy with block vectors), one matrix pass per product (DESIGN.md
// section 24).
//
// Each column is its own restarted GCR solve -- own basis, gammas, betas, alpha, verdict, history and iteration count, the algebra of
// spmv_amd_gcr_solve_device (gcr.hip, steps 1-7 of its header: classical Gram-Schmidt from the q of the product, i ascending in step
// 4, every fma explicit, the breakdown rule, the strict stopping test) element for element. What the columns share is the SpMM
// (spmm_kernels.hip), one dinv[row] per row, and the block application of the preconditioner (launch_mg_multi_term0,
// launch_pcg_multi_cheb_step, mg_cycle_multi: unchanged, they test `done` of PcgMultiColumn records and nothing else, so the solve
// keeps k such records whose `done` every scalar step writes beside its own). Not a block Krylov method: no shared space. All
// running columns are in the same iteration, so they share the slot j = it mod m.
//
// One iteration on the default stream (block vectors interleaved, multi_rhs.hpp; the basis is 2 m block vectors Q_i, Z_i):
//   the application Z = M^-1 R ("none": R itself; "jacobi": the dinv r the x / r kernel left; "chebyshev": term 0, then degree x
//   (SpMM + step); "multigrid": term 0 + the block V-cycle) | the SpMM INTO slot Q_j | multidot: the partials of Q_i.q, i < j, one
//   pass over the basis (not at j = 0) | sums + the betas (not at j = 0) | orthogonalise: step 4 on Q_j in place and on z out of place
//   into Z_j, the partials of q.q and r.q | sums + alpha or the breakdown | the x / r kernel with the partials of r.r ("jacobi": dinv r)
//   | sums + ||r|| and the verdict
// then ONE small blocking read of the k column records: behind the SpMM at most six launches, four at j = 0. A column that has
// converged or broken down is frozen: from the next iteration on no launch changes a bit of its X, R, history, count or record (the
// vector kernels change no bit of it anywhere); its basis slots, Z, D and W are scratch for the SpMM and the application. A NaN or
// inf of one column stays in that column. A launch without a running column returns at once; a unit (one or two neighbouring columns
// of a row) without one reads nothing; a frozen column beside a running one in a 16-byte pair gets its bits back as they came.
//
// Dot products: pcg_multi.hip's shape -- the rounded product per row, the workgroup's 256 rows through block_partials
// (multi_rhs_device.hpp), then the two reduction stages per value and column (4096 partials per slice, then the slice sums) -- so a
// column has the same bits whatever k is and whatever slot it sits in (not the bits of the single solver, whose dots are streaming
// fma chains). Value v of column c and workgroup g lies at partials[(v * k + c) * count + g]. Both stages and the scalar step are ONE
// launch: workgroup (slice, column) sums its slice of every value; with more than one slice it publishes the sums and the workgroup
// that draws the column's last ticket sums them (gcr.hip's hand-over, reduce_device.hpp) and takes the step.
//
// Vector kernels: templated on K = 1..8, the Flat<K> walk (16-byte accesses for even k), every load of a unit -- and of a chunk of
// basis slots -- before the first use, nontemporal loads and stores for streams touched once per pass, plain stores for what the next
// SpMM or application reads. The chunk of basis slots a thread holds in flight (K doubles per block vector and thread): kDotChunk =
// 4 in the multidot, kOrthChunk = 2 (a Q_i and a Z_i unit each) in the orthogonalise kernel -- half the single solver's 8 and 4,
// because a thread carries the K columns of its row: at K = 8 a chunk is 32 doubles in either kernel beside q (8), or q, z, r and the
// kept Z_j (32). The compiler's resource report for gfx950 (-Rpass-analysis=kernel-resource-usage), K = 1 / 2 / 4 / 8: multidot 26 /
// 46 / 76 / 130 VGPRs (8 / 8 / 6 / 3 waves per SIMD), orthogonalise 28 / 48 / 90 / 174 VGPRs (8 / 8 / 5 / 2 waves); 0 scratch bytes
// per lane (no spill) in both at every K = 1 .. 8, no AGPRs. At K = 8 the two waves of a SIMD hold 2 x 64 x (32 + 32) x 8 B = 64 KiB
// of loads per SIMD, past the ~32 KiB per CU that streaming from HBM takes. q's unit is loaded once per thread, the chunks walk the
// basis behind it; a dot's bits do not depend on the chunk it fell into. The multidot sends its values through the one LDS product
// array one by one (three barriers each); sending 2 or 4 values of a chunk through 32 KiB of LDS behind one pair of barriers was
// built, gave the same bits and was SLOWER (3.21 against 3.36 TB/s at slot 15, k = 4): not kept.
//
// Bytes per row and column and iteration on stencil5-csr, kind "none", slot j (only the matrix's 40 B per row are shared): product
// 40 / k + 16, multidot 8 (j + 1), orthogonalise 24 at j = 0 and 32 + 16 j behind it, x / r 48: 128 - 40 (1 - 1 / k) at j = 0,
// 144 + 24 j - 40 (1 - 1 / k) behind it.
//
// This file: the kernels, their launchers, the workspace, the loop and the LAB build's stage hook. What surrounds the loop is
// multi_solve.hpp, shared with the other batched solvers.
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
#include "precond.hpp"
#include "reduce_device.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr const char* kTag = "GCR-MULTI";
constexpr int kMaxRestart = kGcrMultiMaxRestart;
constexpr int kDefaultRestart = 16;
constexpr int kDotChunk = 4;   // basis slots whose units a thread of the multidot kernel holds in flight
constexpr int kOrthChunk = 2;  // basis slots (a Q_i and a Z_i unit each) a thread of the orthogonalise kernel holds in flight

// The basis of one solve: slot i's Q_i = A Z_i (orthogonal per column) and Z_i, an interleaved block vector each. Slots > j are never
// read.
struct GcrMultiBasis {
    double* q[kMaxRestart];
    double* z[kMaxRestart];
};

template <int K>
__device__ __forceinline__ bool any_column_runs(const GcrMultiColumn* __restrict__ cols) {
    bool need = false;
#pragma unroll
    for (int c = 0; c < K; ++c) need = need || cols[c].done == 0;
    return need;
}

// The walk of one workgroup: unit i of this thread is row t of the workgroup, columns col0 .. col0 + V - 1.
#define GCR_MULTI_WALK                            \
    constexpr int V = Flat<K>::V, U = Flat<K>::P; \
    const long long row0 = (long long)blockIdx.x * kBlock
#define GCR_MULTI_UNITS _Pragma("unroll") for (int i = 0; i < U; ++i)
#define GCR_MULTI_UNIT                           \
    const int f = (int)threadIdx.x + kBlock * i; \
    const int t = f / U, col0 = (f - t * U) * V; \
    const long long at = (row0 + t) * K + col0;  \
    const bool inside = row0 + t < n

// R = fma(1.0, b, -1.0 * A x0) (R holds b on entry) ; the partials of r.r ; "jacobi": ZS = dinv r for the first product
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void gcr_multi_init_kernel(long long n, const double* __restrict__ AX, const double* __restrict__ dinv,
                                                               double* __restrict__ R, double* __restrict__ ZS, double* __restrict__ partials,
                                                               long long count) {
    __shared__ double prod[kBlock * K];
    double unused[K] = {};
    GCR_MULTI_WALK;
    GCR_MULTI_UNITS {
        GCR_MULTI_UNIT;
        double r[V] = {};
        if (inside) {
            double ax[V];
            load_unit_once<V>(AX + at, ax);
            load_unit_once<V>(R + at, r);
            const double dv = kJac ? dinv[row0 + t] : 1.0;  // one load per unit: the units of a row read the same 8 bytes
#pragma unroll
            for (int q = 0; q < V; ++q) r[q] = fma(1.0, r[q], -1.0 * ax[q]);
            if (kJac) {
                double h[V];
#pragma unroll
                for (int q = 0; q < V; ++q) h[q] = dv * r[q];
                store_unit_once<V>(R + at, r);
                store_row<V>(ZS + at, h);  // plain: the first SpMM reads it
            } else {
                store_row<V>(R + at, r);  // plain: the first application or SpMM reads it
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = r[q] * r[q];
    }
    unit_partials<K>(prod, true, unused, false, partials, count);
}

// The running columns: the partials of Q_i.q, i = 0 .. j-1 (value i of column c at partials[(i * K + c) * count + g]), q = Q_j. One
// pass over the basis: q's units are loaded once, the basis walks behind them in chunks of kDotChunk slots.
template <int K>
__global__ __launch_bounds__(kBlock) void gcr_multi_multidot_kernel(long long n, const GcrMultiColumn* __restrict__ cols, GcrMultiBasis basis,
                                                                   int j, double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    if (!any_column_runs<K>(cols)) return;  // uniform over the launch
    GCR_MULTI_WALK;
    const double* const qj = basis.q[j];
    double qv[U][V];
    bool run[U][V], live[U];
    GCR_MULTI_UNITS {
        GCR_MULTI_UNIT;
        bool any = false;
#pragma unroll
        for (int q = 0; q < V; ++q) run[i][q] = cols[col0 + q].done == 0, any = any || run[i][q], qv[i][q] = 0.0;
        live[i] = any && inside;
        if (live[i]) load_unit_once<V>(qj + at, qv[i]);
    }
    for (int base = 0; base < j; base += kDotChunk) {
        double av[kDotChunk][U][V];
#pragma unroll
        for (int u = 0; u < kDotChunk; ++u) {  // every load of the chunk before the first use
            const double* const a = basis.q[base + u < j ? base + u : j];
            GCR_MULTI_UNITS {
                GCR_MULTI_UNIT;
                (void)inside;
#pragma unroll
                for (int q = 0; q < V; ++q) av[u][i][q] = 0.0;
                if (live[i] && base + u < j) load_unit_once<V>(a + at, av[u][i]);
            }
        }
#pragma unroll
        for (int u = 0; u < kDotChunk; ++u) {
            if (base + u >= j) break;  // uniform
            GCR_MULTI_UNITS {
                GCR_MULTI_UNIT;
                (void)at, (void)inside;
#pragma unroll
                for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = run[i][q] ? av[u][i][q] * qv[i][q] : 0.0;
            }
            double d[K];
            products_to_rows<K>(prod, d);
            block_partials<K>(d, partials + (long long)(base + u) * K * count, count, blockIdx.x);
            __syncthreads();  // every thread has read its row of prod, and threads < K the wave sums
        }
    }
}

// The running columns: step 4 with i ascending on q = Q_j (in place) and z = z_in (out of place into Z_j), then the partials of q.q
// (value 0) and r.q (value 1). z_in: wherever the application left z -- R itself ("none": loaded once), the "jacobi" block vector, the
// application's Z. At j = 0 z moves into Z_0 and q stays where the SpMM wrote it. A frozen column's Q_j and Z_j keep their bits.
template <int K>
__global__ __launch_bounds__(kBlock) void gcr_multi_orthogonalise_kernel(long long n, const GcrMultiColumn* __restrict__ cols, const double* z_in,
                                                                        GcrMultiBasis basis, int j, const double* R,
                                                                        double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    if (!any_column_runs<K>(cols)) return;  // uniform over the launch
    GCR_MULTI_WALK;
    const bool z_is_r = z_in == R;
    double* const qj = basis.q[j];
    double* const zj = basis.z[j];
    double qv[U][V], zv[U][V], rv[U][V], keep[U][V];
    bool run[U][V], live[U];
    GCR_MULTI_UNITS {
        GCR_MULTI_UNIT;
        bool any = false, all = true;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            run[i][q] = cols[col0 + q].done == 0, any = any || run[i][q], all = all && run[i][q];
            qv[i][q] = zv[i][q] = rv[i][q] = keep[i][q] = 0.0;
        }
        live[i] = any && inside;
        if (live[i]) {
            load_unit_once<V>(qj + at, qv[i]);
            load_unit_once<V>(z_in + at, zv[i]);
            if (!z_is_r) load_unit_once<V>(R + at, rv[i]);
            if (!all) load_unit_once<V>(zj + at, keep[i]);  // a frozen column beside a running one: its bits go back as they came
        }
        if (z_is_r) {
#pragma unroll
            for (int q = 0; q < V; ++q) rv[i][q] = zv[i][q];
        }
    }
    for (int base = 0; base < j; base += kOrthChunk) {
        double av[kOrthChunk][U][V], cv[kOrthChunk][U][V];
#pragma unroll
        for (int u = 0; u < kOrthChunk; ++u) {  // every load of the chunk before the first use
            const int slot = base + u < j ? base + u : 0;
            const double* const a = basis.q[slot];
            const double* const c = basis.z[slot];
            GCR_MULTI_UNITS {
                GCR_MULTI_UNIT;
                (void)inside;
#pragma unroll
                for (int q = 0; q < V; ++q) av[u][i][q] = cv[u][i][q] = 0.0;
                if (live[i] && base + u < j) {
                    load_unit_once<V>(a + at, av[u][i]);
                    load_unit_once<V>(c + at, cv[u][i]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kOrthChunk; ++u) {
            if (base + u >= j) break;  // uniform
            GCR_MULTI_UNITS {
                GCR_MULTI_UNIT;
                (void)at, (void)inside, (void)t;
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    if (!run[i][q]) continue;
                    const double nb = -cols[col0 + q].beta[base + u];
                    qv[i][q] = fma(nb, av[u][i][q], qv[i][q]);
                    zv[i][q] = fma(nb, cv[u][i][q], zv[i][q]);
                }
            }
        }
    }
    double rq[K];
    GCR_MULTI_UNITS {
        GCR_MULTI_UNIT;
        (void)inside;
        if (live[i]) {
            double zz[V];
#pragma unroll
            for (int q = 0; q < V; ++q) zz[q] = run[i][q] ? zv[i][q] : keep[i][q];
            if (j > 0) store_unit_once<V>(qj + at, qv[i]);
            store_unit_once<V>(zj + at, zz);
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            prod[t * K + col0 + q] = run[i][q] ? qv[i][q] * qv[i][q] : 0.0;
            rq[i * V + q] = run[i][q] ? rv[i][q] * qv[i][q] : 0.0;
        }
    }
    unit_partials<K>(prod, true, rq, true, partials, count);
}

// The running columns: x = fma(alpha, z, x) ; r = fma(-alpha, q, r) ; the partials of r.r ; "jacobi": ZS = dinv r for the next SpMM.
// z = Z_j, q = Q_j. A column whose gamma or rho broke down in this iteration is done already: x and r stay as they are.
template <int K, bool kJac>
__global__ __launch_bounds__(kBlock) void gcr_multi_update_xr_kernel(long long n, const GcrMultiColumn* __restrict__ cols,
                                                                    const double* __restrict__ Zj, const double* __restrict__ Qj,
                                                                    const double* __restrict__ dinv, double* __restrict__ X,
                                                                    double* __restrict__ R, double* __restrict__ ZS,
                                                                    double* __restrict__ partials, long long count) {
    __shared__ double prod[kBlock * K];
    if (!any_column_runs<K>(cols)) return;  // uniform over the launch
    double unused[K] = {};
    GCR_MULTI_WALK;
    GCR_MULTI_UNITS {
        GCR_MULTI_UNIT;
        bool run[V], any = false, all = true;
        double alpha[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const GcrMultiColumn& c = cols[col0 + q];
            run[q] = c.done == 0, alpha[q] = c.alpha;
            any = any || run[q], all = all && run[q];
        }
        double r[V] = {};
        if (any && inside) {
            double x[V], z[V], qq[V], keep[V] = {};
            load_unit_once<V>(X + at, x);  // every load of the unit before the first use: one wait
            load_unit_once<V>(Zj + at, z);
            load_unit_once<V>(R + at, r);
            load_unit_once<V>(Qj + at, qq);
            const double dv = kJac ? dinv[row0 + t] : 1.0;
            if (kJac && !all) load_row<V>(ZS + at, keep);  // a frozen column beside a running one: its bits go back as they came
#pragma unroll
            for (int q = 0; q < V; ++q) {
                if (!run[q]) continue;
                x[q] = fma(alpha[q], z[q], x[q]);
                r[q] = fma(-alpha[q], qq[q], r[q]);
            }
            store_unit_once<V>(X + at, x);
            if (kJac) {
                double h[V];
#pragma unroll
                for (int q = 0; q < V; ++q) h[q] = run[q] ? dv * r[q] : keep[q];
                store_unit_once<V>(R + at, r);
                store_row<V>(ZS + at, h);  // plain: the next SpMM reads it
            } else {
                store_row<V>(R + at, r);  // plain: the next application or SpMM reads it
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) prod[t * K + col0 + q] = run[q] ? r[q] * r[q] : 0.0;
    }
    unit_partials<K>(prod, true, unused, false, partials, count);
}
#undef GCR_MULTI_WALK
#undef GCR_MULTI_UNITS
#undef GCR_MULTI_UNIT

// ---- the scalar steps: gcr.hip's gcr_step, per column and branch for branch. which: 0 = r0.r0 ; 1 = the betas of slot j (j values) ;
// 2 = gamma and rho (two values): alpha or the breakdown ; 3 = r.r: ||r|| and the verdict. `stop` of the single solver is `done` here,
// written to the column's shadow record too; steps 1 to 3 pass over a column that is done. ----
__device__ __forceinline__ void gcr_multi_record(GcrMultiColumn& c, double norm, double* hist, int hist_cap) {
    c.iterations += 1;
    c.residual = norm;
    if (c.iterations < hist_cap) hist[c.iterations] = norm;
}

__device__ void gcr_multi_step(GcrMultiColumn& c, PcgMultiColumn& shadow, int which, int j, const double* total, double tol, double* hist,
                               int hist_cap) {
    if (which == 0) {
        for (int i = 0; i < kMaxRestart; ++i) c.gamma[i] = c.beta[i] = 0.0;
        c.alpha = c.rho = 0.0;
        c.b_norm = sqrt(total[0]);
        c.residual = c.b_norm;
        c.done = c.iterations = c.converged = c.breakdown = 0;
        if (hist_cap > 0) hist[0] = c.b_norm;
    } else if (c.done != 0) {
        return;  // frozen: the record keeps its bits
    } else if (which == 1) {
        for (int i = 0; i < j; ++i) c.beta[i] = total[i] / c.gamma[i];
    } else if (which == 2) {
        c.rho = total[1];
        if (usable(total[0]) && usable(total[1])) {
            c.gamma[j] = total[0];
            c.alpha = total[1] / total[0];
        } else {
            c.alpha = 0.0;
            c.breakdown = usable(total[0]) ? 2 : 1, c.done = 1;
            gcr_multi_record(c, c.residual, hist, hist_cap);
        }
    } else {
        const double res = sqrt(total[0]);
        gcr_multi_record(c, res, hist, hist_cap);
        if (res / c.b_norm < tol) c.converged = 1, c.done = 1;
    }
    shadow.done = c.done;
}

// Both reduction stages of nv (1 .. 31) values and the scalar step of column blockIdx.y, in one launch. Workgroup (s, c) sums slice s
// of every value of column c as multi_reduce_slices_kernel does (each thread its strided share in ascending order, then the tree).
// One slice: the same workgroup sums "the slice sums" as the batched step kernels do and takes the step. More: it publishes its sums
// at slices[(v * k + c) * sc + s] and draws a ticket of column c; the workgroup that draws the last one sums them. Steps 1 to 3 lie
// behind a verdict: every workgroup reads `done` before it draws a ticket, and the step writes it only after the last one is drawn.
__global__ __launch_bounds__(kBlock) void gcr_multi_reduce_kernel(const double* __restrict__ partials, long long count, int sc, int k, int nv,
                                                                 unsigned long long* slices, unsigned* tickets, int which, int j, double tol,
                                                                 GcrMultiColumn* cols, PcgMultiColumn* shadow, double* hist, int hist_cap) {
    __shared__ double s[kBlock];
    __shared__ double total[kMaxRestart];
    __shared__ int s_last;
    const int c = (int)blockIdx.y, sl = (int)blockIdx.x;
    if (which >= 1 && cols[c].done != 0) return;  // uniform over the column's workgroups
    const long long lo = (long long)sl * kSlice, hi = lo + kSlice < count ? lo + kSlice : count;
    for (int v = 0; v < nv; ++v) {
        const double* __restrict__ src = partials + ((long long)v * k + c) * count;
        double acc = 0.0;
        for (long long i = lo + threadIdx.x; i < hi; i += kBlock) acc += src[i];
        block_tree(acc, s);
        if (sc == 1) {
            double second = 0.0;
            if (threadIdx.x == 0) second += s[0];
            block_tree(second, s);
            if (threadIdx.x == 0) total[v] = s[0];
        } else if (threadIdx.x == 0) {
            publish(slices + ((long long)v * k + c) * sc + sl, s[0]);
        }
        __syncthreads();
    }
    if (sc > 1) {
        if (threadIdx.x == 0) {
            const unsigned drawn = __hip_atomic_fetch_add(tickets + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = drawn == (unsigned)(sc - 1) ? 1 : 0;
            if (s_last) __hip_atomic_store(tickets + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next reduction
        }
        __syncthreads();
        if (s_last == 0) return;
        for (int v = 0; v < nv; ++v) {
            const unsigned long long* src = slices + ((long long)v * k + c) * sc;
            double acc = 0.0;
            for (int i = (int)threadIdx.x; i < sc; i += kBlock) acc += published(src + i);
            block_tree(acc, s);
            if (threadIdx.x == 0) total[v] = s[0];
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) gcr_multi_step(cols[c], shadow[c], which, j, total, tol, hist + (long long)c * hist_cap, hist_cap);
}

// ---- the loop's launches, one function each: the solve calls these, and so does the LAB build's spmv_amd_gcr_multi_stage ----

// What the launches of one solve (or one stage call) work on.
struct VecArgs {
    bool jac;
    long long n;
    const GcrMultiColumn* cols;
    const double* dinv;
    const double* AX;    // init: A x0
    const double* z_in;  // orthogonalise: where the application left z
    double *X, *R, *ZS;  // ZS: "jacobi", dinv r
    GcrMultiBasis basis;
    int slot;
    double* partials;
    long long count;  // the workgroups of a launch, (n + 255) / 256
};
enum { kStageInit, kStageMultidot, kStageOrth, kStageUpdateXr };

template <int K>
void launch_vec(int stage, const VecArgs& a) {
    const dim3 grid((unsigned)a.count), block(kBlock);
    const int j = a.slot;
    if (stage == kStageMultidot) {
        hipLaunchKernelGGL((gcr_multi_multidot_kernel<K>), grid, block, 0, kBatchStream, a.n, a.cols, a.basis, j, a.partials, a.count);
    } else if (stage == kStageOrth) {
        hipLaunchKernelGGL((gcr_multi_orthogonalise_kernel<K>), grid, block, 0, kBatchStream, a.n, a.cols, a.z_in, a.basis, j, a.R, a.partials,
                           a.count);
    } else if (stage == kStageInit) {
        if (a.jac) hipLaunchKernelGGL((gcr_multi_init_kernel<K, true>), grid, block, 0, kBatchStream, a.n, a.AX, a.dinv, a.R, a.ZS, a.partials, a.count);
        else hipLaunchKernelGGL((gcr_multi_init_kernel<K, false>), grid, block, 0, kBatchStream, a.n, a.AX, a.dinv, a.R, a.ZS, a.partials, a.count);
    } else if (a.jac) {
        hipLaunchKernelGGL((gcr_multi_update_xr_kernel<K, true>), grid, block, 0, kBatchStream, a.n, a.cols, a.basis.z[j], a.basis.q[j], a.dinv, a.X,
                           a.R, a.ZS, a.partials, a.count);
    } else {
        hipLaunchKernelGGL((gcr_multi_update_xr_kernel<K, false>), grid, block, 0, kBatchStream, a.n, a.cols, a.basis.z[j], a.basis.q[j], a.dinv, a.X,
                           a.R, a.ZS, a.partials, a.count);
    }
}

void launch_vector_stage(int k, int stage, const VecArgs& a) {
    auto launch = [&](auto K) { launch_vec<decltype(K)::value>(stage, a); };
    if (!dispatch_k(k, launch)) launch(std::integral_constant<int, kMaxRhs>{});
}

int values_of_step(int which, int j) { return which == 1 ? j : which == 2 ? 2 : 1; }

// The reducing launch behind a group of sums: step `which` of slot j on every column. slices: 32 k x slices_for(count) values;
// tickets: k counters at zero.
void launch_reduce(int k, const double* partials, long long count, double* slices, unsigned* tickets, int which, int j, double tol,
                   GcrMultiColumn* cols, PcgMultiColumn* shadow, double* hist, int hist_cap) {
    const int sc = slices_for(count);
    (void)multi_reduce_slices_kernel;  // multi_rhs_device.hpp's first stage: restated inside the one launch here
    hipLaunchKernelGGL(gcr_multi_reduce_kernel, dim3((unsigned)sc, (unsigned)k), dim3(kBlock), 0, kBatchStream, partials, count, sc, k,
                       values_of_step(which, j), reinterpret_cast<unsigned long long*>(slices), tickets, which, j, tol, cols, shadow, hist, hist_cap);
}

bool fail(const char* what) { return batched_fail(kTag, what); }

// ---- workspace: the batched scaffold's X, R, P ("jacobi": dinv r), AP (the way in and out; the applications' W = A Z), for
// "chebyshev" and "multigrid" D and Z, partials and slices for 32 values, the column records and histories; next to them the 2 m basis
// block vectors, allocated slot by slot, the shadow records and the tickets. Kept between calls, released with the other CG
// workspaces. ----
bool applies(int kind) { return kind == kChebyshev || kind == kMultigrid; }
long long groups_of(int n) { return ((long long)n + kBlock - 1) / kBlock; }
size_t workspace_bytes_of(int n, int k, int restart, int kind) {
    return ((size_t)(4 + (applies(kind) ? 2 : 0) + 2 * restart) * (size_t)n * k + (size_t)kMaxRestart * k * (size_t)groups_of(n)) * sizeof(double);
}

struct GcrMultiWorkspace : BatchedWorkspace<GcrMultiColumn> {
    GcrMultiBasis basis{};
    int slots = 0;
    PcgMultiColumn* shadow = nullptr;
    unsigned* tickets = nullptr;

    GcrMultiWorkspace() : BatchedWorkspace<GcrMultiColumn>(kMaxRestart) {}  // up to 31 betas (or gamma and rho) per column and launch

    void release() {
        for (int i = 0; i < kMaxRestart; ++i) {
            device_release(basis.q[i]);
            device_release(basis.z[i]);
        }
        device_release(shadow);
        device_release(tickets);
        slots = 0;
        BatchedWorkspace<GcrMultiColumn>::release();
    }

    // Sized against free memory before anything is allocated. need: what this request adds; fixed: the part of it that does not grow
    // with the restart; held: basis slots the workspace has already. A request that does not fit names the largest restart that would.
    static bool has_room(size_t need, size_t fixed, int n_, int k_, int restart, int held) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (need <= free_b) return true;
        const size_t per_unit = 2 * (size_t)n_ * k_ * sizeof(double);
        long long fits = held + (free_b > fixed ? (long long)((free_b - fixed) / per_unit) : 0);
        if (fits >= restart) fits = restart - 1;
        char largest[64];
        if (fits >= 1) snprintf(largest, sizeof largest, "restart %lld is the largest that fits", fits);
        else snprintf(largest, sizeof largest, "no restart fits");
        fprintf(stderr, "[%s] the workspace for %d systems of %d rows at restart %d needs %.2f GB more, the device has %.2f GB free: refused (%s)\n",
                kTag, k_, n_, restart, need / 1e9, free_b / 1e9, largest);
        return false;
    }

    bool ensure(int n_, int k_, int device_, int restart, int kind, int hist_cap_) {
        const long long cap = groups_of(n_);
        if (X != nullptr && (n != n_ || k != k_ || device != device_ || partial_cap < cap)) release();
        const size_t vec = (size_t)n_ * k_ * sizeof(double), margin = (size_t)64 << 20;
        const bool dz = applies(kind);
        size_t fixed = margin;
        if (X == nullptr) fixed += workspace_bytes_of(n_, k_, 0, kind) + (size_t)k_ * hist_cap_ * sizeof(double);
        else if (dz && D == nullptr) fixed += 2 * vec;
        const int more = restart > slots ? restart - slots : 0;
        if ((X == nullptr || more > 0 || (dz && D == nullptr)) && !has_room(fixed + 2 * (size_t)more * vec, fixed, n_, k_, restart, slots))
            return false;
        if (!BatchedWorkspace<GcrMultiColumn>::ensure(kTag, n_, k_, device_, cap, hist_cap_, dz)) return false;
        if (shadow == nullptr) {
            shadow = device_try_alloc<PcgMultiColumn>((size_t)k_);
            tickets = device_try_alloc<unsigned>((size_t)kMaxRhs);
            if (!shadow || !tickets) {
                release();
                return fail("the workspace could not be allocated: refused");
            }
            HIP_CHECK(hipMemsetAsync(tickets, 0, kMaxRhs * sizeof(unsigned), kBatchStream));
        }
        for (; slots < restart; ++slots) {
            basis.q[slots] = device_try_alloc<double>((size_t)n_ * k_);
            basis.z[slots] = device_try_alloc<double>((size_t)n_ * k_);
            if (!basis.q[slots] || !basis.z[slots]) {
                release();
                return fail("the basis block vectors could not be allocated: refused");
            }
        }
        return true;
    }
};
GcrMultiWorkspace g_ws;
std::vector<std::vector<double>> g_history;  // of the last batched GCR solve, per column

ColumnSummary summary_of(const GcrMultiColumn& c) {
    static const char* const scalar[] = {nullptr, "gamma = q.q", "rho = r.q", nullptr};
    return {c.iterations, c.converged != 0, c.breakdown != 0, c.residual, c.b_norm, false, scalar[c.breakdown & 3]};
}

}  // namespace

namespace spmv_amd {
void release_gcr_multi_workspace_locked() { g_ws.release(); }
}  // namespace spmv_amd

extern "C" size_t spmv_amd_gcr_multi_workspace_bytes(int rows, int nrhs, int restart, const char* kind) {
    const int kd = kind_of(kind);
    if (rows < 1 || nrhs < 1 || nrhs > kMaxRhs || restart < 0 || restart > kMaxRestart || kd < 0) return 0;
    return workspace_bytes_of(rows, nrhs, restart == 0 ? kDefaultRestart : restart, kd);
}

extern "C" int spmv_amd_gcr_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int restart, int nrhs,
                                               const double* B, double* X, const CGConfig* config, CGStats* stats) {
    // argument checks: all before the first HIP call
    if (op == nullptr || m == nullptr) return fail("null argument"), 1;  // the two pointers the shared checks do not name so
    if (!check_rhs(kTag, nrhs)) return 1;
    if (restart < 0 || restart > kMaxRestart) {
        fprintf(stderr, "[%s] restart = %d: 1 .. %d, or 0 for the default %d: refused\n", kTag, restart, kMaxRestart, kDefaultRestart);
        return 1;
    }
    MultiOperand o;
    if (!check_batched_system(kTag, kTag, op, mat, nrhs, B, X, config, stats, &o)) return 1;
    // kind "multigrid": a hierarchy with block vectors (spmv_amd_precond_create_multigrid_multi, ..._multigrid3d_multi) of at least nrhs columns
    const bool mg = m->kind == kMultigrid, cheb = m->kind == kChebyshev, jac = m->kind == kJacobi;
    const int capacity = mg ? mg_multi_capacity(mg_multi_of(m->mg)) : 0;
    if (mg && capacity == 0)
        return fail("kind 'multigrid' keeps single vectors on every level of its hierarchy: not available for several right-hand sides, refused"), 1;
    if (mg && nrhs > capacity) {
        fprintf(stderr, "[%s] nrhs = %d, the multigrid preconditioner's hierarchy holds block vectors of max_rhs = %d columns: refused\n", kTag, nrhs,
                capacity);
        return 1;
    }
    if (!mg && !cheb && !jac && m->kind != kNone) return fail("unknown preconditioner kind: refused"), 1;
    if (m->n != mat->rows) {
        fprintf(stderr, "[%s] the preconditioner is for %d rows, mat->rows = %d\n", kTag, m->n, mat->rows);
        return 1;
    }
    if (!precond_matches(op, m, diagonal_source_of(op))) return fail("the preconditioner does not belong to this operator as it stands: refused"), 1;
    const int n = mat->rows, k = nrhs;
    const int mr = restart == 0 ? kDefaultRestart : restart;
    const CGConfig cfg = *config;

    CgWorkspaceScope scope;
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    const long long vec_count = groups_of(n);
    GcrMultiWorkspace& w = g_ws;
    if (!w.ensure(n, k, device, mr, m->kind, cfg.max_iters + 1)) return 1;
    load_block_system(w, k, n, B, X, true);  // the records as zeros: done = 0
    HIP_CHECK(hipMemsetAsync(w.shadow, 0, (size_t)k * sizeof(PcgMultiColumn), kBatchStream));  // so the first application's launches run

    std::vector<ColumnSummary> cols;
    StageTimers T(cfg.enable_detailed_timers != 0, kBatchStream);
    VecArgs a{};
    a.jac = jac, a.n = n, a.cols = w.cols, a.dinv = jac ? m->dinv : nullptr, a.X = w.X, a.R = w.R, a.ZS = jac ? w.P : nullptr;
    a.basis = w.basis, a.partials = w.partials, a.count = vec_count;
    auto vec = [&](int stage, int j) {
        a.slot = j;
        T.run(&T.t_blas, [&] { launch_vector_stage(k, stage, a); });
    };
    auto reduce = [&](int which, int j) {
        T.run(&T.t_red, [&] {
            launch_reduce(k, w.partials, vec_count, w.slices, w.tickets, which, j, cfg.tolerance, w.cols, w.shadow, w.hist, w.hist_cap);
        });
    };
    auto spmm = [&](const double* in, double* out) { T.run(&T.t_spmv, [&] { launch_spmm(o.plan, k, in, out, nullptr, kBatchStream); }); };
    // step 1: where Z = M^-1 R is once the application's launches are enqueued. Level 0 of the cycle and the Chebyshev steps work on
    // D, Z and the AP buffer (W = A Z); every launch of an application tests the shadow records.
    auto apply = [&]() -> const double* {
        if (jac) return w.P;
        if (!mg && !cheb) return w.R;
        const double c0 = mg ? m->mg->levels[0].coef[0] : m->coef[0];
        T.run(&T.t_blas, [&] { launch_mg_multi_term0(k, n, w.shadow, w.R, m->dinv, c0, w.D, w.Z); });
        if (mg) mg_cycle_multi(m->mg, k, w.shadow, w.R, w.D, w.Z, w.AP, w.partials, vec_count, &T);
        for (int s = 1; cheb && s <= m->degree; ++s) {
            spmm(w.Z, w.AP);
            T.run(&T.t_blas, [&] {
                launch_pcg_multi_cheb_step(k, n, w.shadow, w.AP, w.R, m->dinv, m->coef[2 * s], m->coef[2 * s - 1], w.D, w.Z, 0, nullptr, vec_count);
            });
        }
        return w.Z;
    };
    // what print_iteration asks of a column: it took part in the iteration just read when it was running before it
    std::vector<char> was_running;
    auto read = [&] {
        was_running.assign((size_t)k, 0);
        for (size_t j = 0; j < cols.size(); ++j) was_running[j] = !(cols[j].converged || cols[j].breakdown);
        read_columns(w, k, summary_of, cols);
        for (int j = 0; j < k; ++j) cols[(size_t)j].active = was_running[(size_t)j] != 0;
    };

    T.total.begin(kBatchStream);
    a.AX = w.AP;
    spmm(w.X, w.AP);  // A x0 into the AP buffer, free from here to the way out
    vec(kStageInit, 0);
    reduce(0, 0);
    read();
    if (cfg.verbose >= 1) print_initial_residuals(kTag, cols, spmv_amd_precond_kind(m));
    for (int it = 0; it < cfg.max_iters && any_column_running(cols); ++it) {
        const int j = it % mr;
        a.z_in = apply();
        spmm(a.z_in, w.basis.q[j]);  // Q_j = A Z for all columns; a frozen column's slot is scratch
        if (j > 0) {
            vec(kStageMultidot, j);
            reduce(1, j);  // the betas
        }
        vec(kStageOrth, j);
        reduce(2, j);  // gamma, rho, alpha -- or the breakdown
        vec(kStageUpdateXr, j);
        reduce(3, j);  // ||r|| and the verdict
        read();        // synchronises: the one blocking read of the iteration
        if (cfg.verbose >= 2) print_iteration(kTag, cols);
    }
    T.total.end(kBatchStream);
    finish_batched_solve(kTag, w, k, n, X, stats, cfg, T, T.total.elapsed_ms(), cols, g_history);
    return 0;
}

extern "C" int spmv_amd_gcr_last_history_multi(int column, double* out, int cap) {
    if (column < 0 || column >= (int)g_history.size()) return -1;
    return copy_history(g_history[(size_t)column], out, cap);
}

#ifdef SPMV_AMD_LAB
// ---- the loop's kernels one stage at a time on caller data (include/spmv_amd/lab.h; tests/test_gcr_multi_stages_gpu.py) ----
static_assert(sizeof(SpmvAmdGcrMultiColumn) == sizeof(GcrMultiColumn) && offsetof(SpmvAmdGcrMultiColumn, beta) == offsetof(GcrMultiColumn, beta) &&
                  offsetof(SpmvAmdGcrMultiColumn, alpha) == offsetof(GcrMultiColumn, alpha) &&
                  offsetof(SpmvAmdGcrMultiColumn, rho) == offsetof(GcrMultiColumn, rho) &&
                  offsetof(SpmvAmdGcrMultiColumn, b_norm) == offsetof(GcrMultiColumn, b_norm) &&
                  offsetof(SpmvAmdGcrMultiColumn, residual) == offsetof(GcrMultiColumn, residual) &&
                  offsetof(SpmvAmdGcrMultiColumn, done) == offsetof(GcrMultiColumn, done) &&
                  offsetof(SpmvAmdGcrMultiColumn, iterations) == offsetof(GcrMultiColumn, iterations) &&
                  offsetof(SpmvAmdGcrMultiColumn, converged) == offsetof(GcrMultiColumn, converged) &&
                  offsetof(SpmvAmdGcrMultiColumn, breakdown) == offsetof(GcrMultiColumn, breakdown),
              "lab.h's column record is the device record, field for field");
static_assert(SPMV_AMD_GCR_MAX_RESTART == kMaxRestart && SPMV_AMD_GCR_MULTI_DOT_CHUNK == kDotChunk && SPMV_AMD_GCR_MULTI_ORTH_CHUNK == kOrthChunk,
              "lab.h states the solver's restart limit and chunk sizes");

extern "C" int spmv_amd_gcr_multi_stage(const char* stage, const char* kind, int k, SpmvAmdGcrMultiStageArgs* a) {
    // argument checks: all before the first HIP call. 16: a block vector the vector kernels access in 16-byte pairs
    static const char* const kStages = "init, multidot, orthogonalise, update_xr, reduce";
    char names[96];
    auto refuse = [&](const char* what) { return stage_fail(kTag, stage, what); };
    auto pointer = [&](const char* name, const void* ptr, int align) { return stage_pointer(kTag, stage, name, ptr, align); };
    int st;
    if (stage == nullptr) {
        snprintf(names, sizeof names, "no stage named (%s)", kStages);
        return refuse(names), 1;
    }
    if (!strcmp(stage, "init")) st = kStageInit;
    else if (!strcmp(stage, "multidot")) st = kStageMultidot;
    else if (!strcmp(stage, "orthogonalise")) st = kStageOrth;
    else if (!strcmp(stage, "update_xr")) st = kStageUpdateXr;
    else if (!strcmp(stage, "reduce")) st = -1;
    else {
        snprintf(names, sizeof names, "unknown stage (%s)", kStages);
        return refuse(names), 1;
    }
    if (k < 1 || k > kMaxRhs) return refuse("k is not 1 to 8"), 1;
    if (a == nullptr) return refuse("null arguments"), 1;
    bool jac = false;
    GcrMultiBasis basis{};
    if (st == -1) {
        if (a->count < 1) return refuse("count < 1"), 1;
        if (a->which < 0 || a->which > 3) return refuse("which is not 0, 1, 2 or 3"), 1;
        if (a->which == 1 && (a->slot < 1 || a->slot >= kMaxRestart)) return refuse("slot outside 1 .. 31"), 1;
        if (a->which == 2 && (a->slot < 0 || a->slot >= kMaxRestart)) return refuse("slot outside 0 .. 31"), 1;
        if (a->hist_cap < 0) return refuse("hist_cap < 0"), 1;
        if (!pointer("partials", a->partials, 8) || !pointer("cols", a->cols, 8) || !pointer("shadow", a->shadow, 8)) return 1;
        if (a->hist_cap > 0 && !pointer("hist", a->hist, 8)) return 1;
    } else {
        if (st == kStageInit || st == kStageUpdateXr) {
            const int kd = kind_of(kind);
            if (kd != kNone && kd != kJacobi) return refuse("unknown preconditioner kind (none, jacobi)"), 1;
            jac = kd == kJacobi;
        }
        if (a->n < 1 || a->n > (size_t)INT_MAX) return refuse("n < 1 or beyond the solver's int rows"), 1;
        if (st != kStageInit) {
            const int lo = st == kStageMultidot ? 1 : 0;
            if (a->slot < lo || a->slot >= kMaxRestart) return refuse(st == kStageMultidot ? "slot outside 1 .. 31" : "slot outside 0 .. 31"), 1;
            if (!pointer("cols", a->cols, 8)) return 1;
            if (a->Q == nullptr) return refuse("Q is null"), 1;
            if (st != kStageMultidot && a->Z == nullptr) return refuse("Z is null"), 1;
            const int j = a->slot;
            char name[16];
            for (int i = st == kStageUpdateXr ? j : 0; i <= j; ++i) {  // slots > j are not looked at
                snprintf(name, sizeof name, "Q[%d]", i);
                if (!pointer(name, a->Q[i], 16)) return 1;
                basis.q[i] = a->Q[i];
                if (st == kStageMultidot) continue;
                snprintf(name, sizeof name, "Z[%d]", i);
                if (!pointer(name, a->Z[i], 16)) return 1;
                basis.z[i] = a->Z[i];
            }
        }
        if (jac && (!pointer("dinv", a->dinv, 8) || !pointer("ZS", a->ZS, 16))) return 1;
        if (!pointer("partials", a->partials, 8)) return 1;
        if (st != kStageMultidot && !pointer("R", a->R, 16)) return 1;
        if (st == kStageInit && !pointer("AX", a->AX, 16)) return 1;
        if (st == kStageOrth && !pointer("z_in", a->z_in, 16)) return 1;
        if (st == kStageUpdateXr && !pointer("X", a->X, 16)) return 1;
    }

    GcrMultiColumn* cols = reinterpret_cast<GcrMultiColumn*>(a->cols);
    double* slices = nullptr;
    unsigned* tickets = nullptr;
    if (st == -1) {
        slices = device_alloc<double>((size_t)kMaxRestart * k * slices_for(a->count));
        tickets = device_alloc<unsigned>((size_t)kMaxRhs);
        HIP_CHECK(hipMemsetAsync(tickets, 0, kMaxRhs * sizeof(unsigned), kBatchStream));
        launch_reduce(k, a->partials, a->count, slices, tickets, a->which, a->slot, a->tol, cols, reinterpret_cast<PcgMultiColumn*>(a->shadow), a->hist,
                      a->hist_cap);
    } else {
        VecArgs v{};
        v.jac = jac, v.n = (long long)a->n, v.cols = cols, v.dinv = a->dinv, v.AX = a->AX, v.z_in = a->z_in, v.X = a->X, v.R = a->R, v.ZS = a->ZS;
        v.basis = basis, v.slot = st == kStageInit ? 0 : a->slot, v.partials = a->partials;
        v.count = groups_of((int)a->n);
        launch_vector_stage(k, st, v);
        a->count = v.count;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    device_release(slices);
    device_release(tickets);
    return 0;
}
#endif  // SPMV_AMD_LAB
