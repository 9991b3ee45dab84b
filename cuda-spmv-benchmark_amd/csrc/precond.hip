// precond.hip -- the preconditioner record (precond.hpp) of every solver that takes one: kinds "none" and "jacobi" (DESIGN.md section
// 13), a Chebyshev polynomial in D^-1 A (section 14); kind "multigrid" is made by multigrid.hip, multigrid3d.hip and amg.hip on the
// passes below. Here: the set-up passes (diagonal, Gershgorin bound), the creators with their one operator check (creation_source) and
// the one sentence about a bad diagonal row (inverse_diagonal), the Chebyshev coefficients, the runner of a Chebyshev step (cheb_step,
// the only place that chooses its form from a ChebSpmv; pcg.hip's header has the forms), what every entry point checks of an (operator,
// preconditioner) pair (precond_matches), one application on its own (spmv_amd_precond_apply_device), info and destroy. The
// preconditioned loop is pcg.hip; its term-0 kernel and its reduce launch are reached through precond.hpp. Everything here speaks
// behind [PCG], the tag the record was born under.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "precond.hpp"
#include "reduce_device.hpp"
#include "single_solve.hpp"
#include "stream_device.hpp"

using namespace spmv_amd;

namespace {

bool fail(const char* what) {
    fprintf(stderr, "[PCG] %s\n", what);
    return false;
}

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

// ---- kind "chebyshev": lambda_max, the streaming step ----

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

bool spmv_amd::cheb_after_term0(const SpmvAmdPrecond* m, ChebRun& c) {
    c.rz_partials = c.partials + stream_grid(c.n), c.rz_count = (int)stream_grid(c.n);
    return cheb_steps(c, m->degree, m->coef, true);
}

namespace {

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

extern "C" SpmvAmdPrecond* spmv_amd_precond_create(SpmvOperator* op, const char* kind, int* bad_row) {
    if (bad_row != nullptr) *bad_row = -1;
    const int k = kind_of(kind);
    if (k != kNone && k != kJacobi) {
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

// the set-up passes and the creators' operator check for multigrid.hip, multigrid3d.hip and amg.hip (precond.hpp)
namespace spmv_amd {
double* inverse_diagonal_of_csr(const SlabCsr& m, int n, const char* who, int* bad_row) {
    return inverse_diagonal(0, m, nullptr, nullptr, 0, n, who, bad_row);
}
double gershgorin_of_csr(const SlabCsr& m, int n, const double* dinv) { return gershgorin_bound(0, m, nullptr, nullptr, 0, n, dinv); }
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
            launch_cheb_term0_apply(n, d_r, m->dinv, m->coef[0], cd, c.z, m->degree == 0, partials);
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
