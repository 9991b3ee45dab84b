// amg.hip -- aggregation AMG for the general CSR operator "cusparse-csr" (include/spmv_amd/api.h states the
// algebra down to the order of every sum): a handle of kind "multigrid" whose hierarchy is made from the matrix, not from a grid.
//
// Set-up: the creator reads the operator's device CSR back, runs amg_setup.hpp level by level on the host -- strong couplings, three
// aggregation passes, member lists, the Galerkin product --, sizes the whole hierarchy against free device memory, uploads each
// level and runs precond.hpp's device passes on it (inverse_diagonal_of_csr, gershgorin_of_csr). The set-up is sequential by
// definition (aggregates are numbered in order of creation) and its wall time is reported (spmv_amd_precond_amg_info).
//
// Cycle: multigrid.hip's CycleOps on mg_schedule.hpp's mg_vcycle, as for the geometric hierarchies. A level here has dim == 0:
// level 0 runs the operator's own run_device, every other level launch_csr_spmv in csr_auto_variant of its matrix, both followed
// by precond.hip's streaming step; the two transfers are the kernels below.
//
// spmv_amd_precond_create_amg_multi is the same creator: its hierarchy also holds multigrid_multi.hip's block
// vectors and SpMM plans, and the batched cycle's two transfers are amg_multi.hip's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "amg_setup.hpp"
#include "multi_rhs.hpp"
#include "multigrid.hpp"
#include "stream_device.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators, pcg.hip and multigrid.hip
constexpr int kWave = 64;
constexpr int kGroup = 8;  // lanes per aggregate: eight aggregates per wave
constexpr int kMaxSmoother = 8;

bool fail(const char* what) {
    fprintf(stderr, "[PCG] amg: %s\n", what);
    return false;
}

// ---- residual + restriction in one launch: r_c = P^T (r - A z), A z and r - A z never stored ----
// One-wave workgroups; eight lanes per aggregate, so a wave owns eight consecutive aggregates. Per round every lane of a group takes
// one member row (members[m0 + 8 round + sub]) and walks its CSR entries as ONE sequential chain s = +0.0 ; s = fma(v[k], z[col[k]], s)
// for ascending k -- the chain of the stream and row-scalar products, whatever variant the level's product runs --, then
// t = fma(-1.0, s, r[row]). Behind the round the eight t travel through __shfl and are added in member order: acc = t_m0 for the
// first, acc = acc + t after it; all eight lanes of a group hold the same acc, lane 0 of the group stores it. The number of rounds is
// the maximum over the wave's eight groups, so every lane of the wave runs the same rounds and the shuffles sit in uniform control
// flow: a lane without a row in a round takes part and contributes nothing (its t is not added: the sum skips it by count, not by
// value). An aggregate of thousands of members (a hub row's) loops; no LDS, no scratch.
// Bytes per fine row of a level with q entries per row: 12 q of matrix (8 value + 4 column), 8 of row pointer (both ends: member rows
// are not neighbours), 8 of r, 4 of member index and the gathered z -- 8 q requested, 8 unique where the cache holds the neighbours --
// plus 8 + 4 per aggregate (r_c, agg_ptr): 12 q + 28 + 8 q gathered. A stored and re-read t would add 16.
__global__ __launch_bounds__(kWave) void amg_residual_restrict_kernel(SlabCsr m, int coarse_rows, const int* __restrict__ agg_ptr,
                                                                      const int* __restrict__ members, const double* __restrict__ z,
                                                                      const double* __restrict__ r, double* __restrict__ rc) {
    const int lane = (int)threadIdx.x;
    const int sub = lane & (kGroup - 1), first = lane & ~(kGroup - 1);
    const long long I = (long long)blockIdx.x * (kWave / kGroup) + (lane / kGroup);
    const bool live = I < coarse_rows;
    const int m0 = live ? agg_ptr[I] : 0, m1 = live ? agg_ptr[I + 1] : 0;
    int rounds = (m1 - m0 + kGroup - 1) / kGroup;
#pragma unroll
    for (int off = kWave / 2; off >= kGroup; off >>= 1) {  // the wave's maximum: the lanes of a group agree already
        const int other = __shfl_xor(rounds, off);
        rounds = other > rounds ? other : rounds;
    }
    double acc = 0.0;
    for (int round = 0; round < rounds; ++round) {
        const int begin = m0 + kGroup * round;
        const int have = m1 - begin;  // members of this round: may be <= 0 in a group that is done
        double t = 0.0;
        if (sub < have) {
            const int row = members[begin + sub];
            double s = 0.0;
            for (int k = m.row_ptr[row]; k < m.row_ptr[row + 1]; ++k) s = fma(m.values[k], z[m.col_idx[k]], s);
            t = fma(-1.0, s, r[row]);
        }
#pragma unroll
        for (int q = 0; q < kGroup; ++q) {
            const double tq = __shfl(t, first + q);
            const double sum = (round == 0 && q == 0) ? tq : acc + tq;
            acc = q < have ? sum : acc;
        }
    }
    if (live && sub == 0) rc[I] = acc;  // plain: the next level reads it at once
}

// ---- prolongation + correction: z = fma(2.0, e_c[agg[i]], z), z in place; streaming, one-wave workgroups, a 16-byte pair per lane ----
__global__ __launch_bounds__(kWave) void amg_prolong_correct_kernel(size_t rows, const int* __restrict__ agg, const double* __restrict__ ec,
                                                                    double* __restrict__ z) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < (rows >> 1)) {
        d2 zv = reinterpret_cast<const d2*>(z)[i];
        zv.x = fma(2.0, ec[agg[2 * i]], zv.x);
        zv.y = fma(2.0, ec[agg[2 * i + 1]], zv.y);
        reinterpret_cast<d2*>(z)[i] = zv;  // plain: the post-smoother's product reads it
    }
    if ((rows & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[rows - 1] = fma(2.0, ec[agg[rows - 1]], z[rows - 1]);
}

}  // namespace

// ---- the launches (multigrid.hpp) ----
namespace spmv_amd {

void launch_amg_residual_restrict(const SlabCsr& m, int coarse_rows, const int* agg_ptr, const int* members, const double* z, const double* r,
                                  double* rc) {
    if (coarse_rows <= 0) return;
    const unsigned grid = (unsigned)(((long long)coarse_rows + kWave / kGroup - 1) / (kWave / kGroup));
    hipLaunchKernelGGL(amg_residual_restrict_kernel, dim3(grid), dim3(kWave), 0, kStream, m, coarse_rows, agg_ptr, members, z, r, rc);
}

void launch_amg_prolong_correct(size_t rows, const int* agg, const double* ec, double* z) {
    if (rows == 0) return;
    hipLaunchKernelGGL(amg_prolong_correct_kernel, dim3(stream_grid(rows)), dim3(kWave), 0, kStream, rows, agg, ec, z);
}

}  // namespace spmv_amd

namespace {

template <class T>
T* uploaded(const std::vector<T>& host) {
    T* p = device_try_alloc<T>(host.size());
    if (p != nullptr) upload(p, host.data(), host.size());
    return p;
}

// Uploads level l of the host hierarchy (l > 0: its matrix; every level but the coarsest: its aggregates), runs the device passes on
// it and allocates its vectors; false = refused (said on stderr).
bool finish_level(MgHierarchy* h, int l, const amg::HostLevel& H, int* bad_row) {
    MgLevel& L = h->levels[(size_t)l];
    const bool coarsest = l + 1 == (int)h->levels.size();
    if (l > 0) {
        L.A.allocate((size_t)L.rows, (size_t)H.A.nnz());
        upload(L.A.row_ptr, H.A.row_ptr.data(), H.A.row_ptr.size());
        upload(L.A.col_idx, H.A.col_idx.data(), H.A.col_idx.size());
        upload(L.A.values, H.A.values.data(), H.A.values.size());
        SlabCsr v;
        v.row_ptr = L.A.row_ptr, v.col_idx = L.A.col_idx, v.values = L.A.values;
        v.n_local = v.n_global = L.rows;
        v.nnz_local = H.A.nnz();
        v.max_row_nnz = H.A.max_row_nnz();
        L.A.view = L.view = v;
        L.csr_variant = csr_auto_variant(L.view);
        char who[40];
        snprintf(who, sizeof who, "amg: level %d", l);
        L.dinv = inverse_diagonal_of_csr(L.view, L.rows, who, bad_row);
        if (L.dinv == nullptr) return false;
    }
    if (!coarsest) {
        L.coarse_rows = H.g.count, L.max_aggregate = H.g.max_aggregate;
        L.agg = uploaded(H.g.agg), L.agg_ptr = uploaded(H.g.agg_ptr), L.members = uploaded(H.g.members);
        if (L.agg == nullptr || L.agg_ptr == nullptr || L.members == nullptr) return fail("the aggregates could not be allocated: refused");
    }
    L.lambda_max = gershgorin_of_csr(L.view, L.rows, L.dinv);
    const double lmin = coarsest ? L.lambda_max / 30.0 : L.lambda_max / 4.0;
    if (!isfinite(L.lambda_max) || !(lmin > 0.0) || !(lmin < L.lambda_max)) {
        fprintf(stderr, "[PCG] amg: level %d: the interval [%g, %g] is not 0 < lambda_min < lambda_max, both finite: refused\n", l, lmin,
                L.lambda_max);
        return false;
    }
    L.degree = coarsest ? kMgCoarsestDegree : h->smoother_degree;
    chebyshev_coefficients(L.degree, lmin, L.lambda_max, L.coef);
    if (l > 0) L.r = device_try_alloc<double>((size_t)L.rows);
    L.d = device_try_alloc<double>((size_t)L.rows);
    L.z = device_try_alloc<double>((size_t)L.rows);
    L.aux = device_try_alloc<double>((size_t)L.rows);
    if ((l > 0 && L.r == nullptr) || L.d == nullptr || L.z == nullptr || L.aux == nullptr) return fail("the level vectors could not be allocated: refused");
    return true;
}

// The one creator. multi false: spmv_amd_precond_create_amg (max_rhs is 0 and not looked at); true (..._amg_multi): max_rhs is checked
// beside the other arguments, and the hierarchy also gets block vectors of that many columns and an SpMM plan on every level
// (multigrid_multi.hip's mg_multi_create).
SpmvAmdPrecond* create_amg(SpmvOperator* op, int smoother_degree, int max_levels, double strength, int max_rhs, bool multi, int* bad_row) {
    const auto started = std::chrono::steady_clock::now();
    // argument checks: all before the first HIP call
    if (bad_row != nullptr) *bad_row = -1;
    if (op == nullptr) return fail("null operator"), nullptr;
    if (smoother_degree < 0 || smoother_degree > kMaxSmoother) {
        fprintf(stderr, "[PCG] amg: smoother degree %d is outside 0..%d: refused\n", smoother_degree, kMaxSmoother);
        return nullptr;
    }
    if (max_levels < 0 || max_levels > amg::kMaxLevels) {
        fprintf(stderr, "[PCG] amg: max_levels %d is neither 0 (automatic) nor 1..%d: refused\n", max_levels, amg::kMaxLevels);
        return nullptr;
    }
    if (!isfinite(strength) || !(strength >= 0.0) || !(strength < 1.0)) {
        fprintf(stderr, "[PCG] amg: strength %g is not a finite number in [0, 1): refused\n", strength);
        return nullptr;
    }
    if (multi && (max_rhs < 1 || max_rhs > kMaxRhs)) {
        fprintf(stderr, "[PCG] amg: max_rhs %d is outside 1..%d: refused\n", max_rhs, kMaxRhs);
        return nullptr;
    }
    const DiagonalSource d = diagonal_source_of(op);
    if (d.owner == nullptr || d.kind != DiagonalSource::Csr || op->name == nullptr || strcmp(op->name, "cusparse-csr") != 0) {
        fprintf(stderr,
                "[PCG] amg: operator '%s' is not cusparse-csr (stencil5-csr and stencil7-csr have creators of their own; load the same matrix "
                "into cusparse-csr to compare): refused\n",
                op->name ? op->name : "?");
        return nullptr;
    }
    if (!d.ready) {
        fprintf(stderr, "[PCG] operator '%s' used before init\n", op->name);
        return nullptr;
    }
    if (d.rows != d.cols || d.rows < 1 || d.csr.row_offset != 0 || d.csr.n_local != d.rows) {
        fprintf(stderr, "[PCG] operator '%s' holds a %d x %d matrix: a square one is required\n", op->name, d.rows, d.cols);
        return nullptr;
    }

    // the host hierarchy: no device memory is taken before its size is known
    amg::HostCsr A0;
    A0.row_ptr.resize((size_t)d.rows + 1);
    A0.col_idx.resize((size_t)d.csr.nnz_local);
    A0.values.resize((size_t)d.csr.nnz_local);
    HIP_CHECK(hipStreamSynchronize(kStream));
    download(A0.row_ptr.data(), d.csr.row_ptr, A0.row_ptr.size());
    download(A0.col_idx.data(), d.csr.col_idx, A0.col_idx.size());
    download(A0.values.data(), d.csr.values, A0.values.size());
    for (const int c : A0.col_idx)
        if (c < 0 || c >= d.rows) return fail("a column index of the operator's matrix lies outside the matrix: refused"), nullptr;
    std::vector<amg::HostLevel> host = amg::hierarchy(std::move(A0), strength, max_levels);

    MgHierarchy* h = new MgHierarchy();
    h->dim = 0;
    h->smoother_degree = smoother_degree;
    h->strength = strength;
    size_t need = 0;
    for (size_t l = 0; l < host.size(); ++l) {
        MgLevel L;
        L.dim = 0, L.n = 0, L.rows = host[l].A.rows();
        h->levels.push_back(L);
        need += (size_t)L.rows * sizeof(double) * (l == 0 ? 3 : 5);
        if (l > 0) need += (size_t)host[l].A.nnz() * (sizeof(double) + sizeof(int)) + ((size_t)L.rows + 1) * sizeof(int) + 3 * 4096;
        if (l + 1 < host.size()) need += (2 * (size_t)L.rows + (size_t)host[l].g.count + 1) * sizeof(int);
    }
    if (multi) need += mg_multi_bytes(h, max_rhs);
    SpmvAmdPrecond* pm = nullptr;
    char what[64];
    snprintf(what, sizeof what, "%d levels on %d rows (amg)", (int)h->levels.size(), d.rows);
    bool ok = device_has_room(need + (size_t)d.rows * sizeof(double) + ((size_t)64 << 20), "PCG", what);
    if (ok) {
        MgLevel& top = h->levels[0];
        top.view = d.csr;
        top.op = op;
        top.own_dinv = false;
        top.dinv = inverse_diagonal_of_csr(top.view, top.rows, "amg: level 0", bad_row);
        if (top.dinv == nullptr) {
            ok = false;
        } else {
            pm = new SpmvAmdPrecond();
            pm->kind = kMultigrid;
            pm->n = d.rows;
            pm->dinv = top.dinv;
            pm->degree = smoother_degree;
            pm->owner = d.owner;
            pm->generation = d.generation;
        }
    }
    for (int l = 0; ok && l < (int)h->levels.size(); ++l) ok = finish_level(h, l, host[(size_t)l], bad_row);
    if (ok) {
        h->partials = device_try_alloc<double>((size_t)stream_grid((size_t)h->levels[0].rows));
        if (h->partials == nullptr) ok = fail("the partials could not be allocated: refused");
    }
    if (ok && multi) {
        h->multi = mg_multi_create(h, max_rhs);
        ok = h->multi != nullptr;
    }
    HIP_CHECK(hipStreamSynchronize(kStream));
    if (!ok) {
        mg_destroy(h);
        if (pm != nullptr) {
            device_release(pm->dinv);
            delete pm;
        }
        return nullptr;
    }
    pm->mg = h;
    pm->lambda_max = h->levels[0].lambda_max;
    pm->lambda_min = pm->lambda_max / (h->levels.size() == 1 ? 30.0 : 4.0);
    h->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count();
    return pm;
}

}  // namespace

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_amg(SpmvOperator* op, int smoother_degree, int max_levels, double strength, int* bad_row) {
    return create_amg(op, smoother_degree, max_levels, strength, 0, false, bad_row);
}

extern "C" SpmvAmdPrecond* spmv_amd_precond_create_amg_multi(SpmvOperator* op, int smoother_degree, int max_levels, double strength, int max_rhs,
                                                             int* bad_row) {
    return create_amg(op, smoother_degree, max_levels, strength, max_rhs, true, bad_row);
}

extern "C" int spmv_amd_precond_amg_info(const SpmvAmdPrecond* m, int* levels, int* smoother_degree, double* strength, int* rows, long long* nnz,
                                         int* max_aggregate, double* lambda_max, double* setup_ms, int cap) {
    if (m == nullptr || m->kind != kMultigrid || m->mg == nullptr || m->mg->dim != 0) return 0;
    const MgHierarchy& h = *m->mg;
    const int count = h.count();
    if (levels != nullptr) *levels = count;
    if (smoother_degree != nullptr) *smoother_degree = h.smoother_degree;
    if (strength != nullptr) *strength = h.strength;
    if (setup_ms != nullptr) *setup_ms = h.setup_ms;
    for (int l = 0; l < count && l < cap; ++l) {
        const MgLevel& L = h.levels[(size_t)l];
        if (rows != nullptr) rows[l] = L.rows;
        if (nnz != nullptr) nnz[l] = L.nnz();
        if (max_aggregate != nullptr) max_aggregate[l] = L.max_aggregate;
        if (lambda_max != nullptr) lambda_max[l] = L.lambda_max;
    }
    return count;
}

#ifdef SPMV_AMD_LAB
extern "C" int spmv_amd_precond_amg_level_aggregates(const SpmvAmdPrecond* m, int level, int* agg) {
    if (m == nullptr || m->kind != kMultigrid || m->mg == nullptr || m->mg->dim != 0) return fail("level_aggregates: not an AMG preconditioner"), 1;
    if (level < 0 || level + 1 >= m->mg->count()) return fail("level_aggregates: no such level, or the coarsest one"), 1;
    const MgLevel& L = m->mg->levels[(size_t)level];
    HIP_CHECK(hipStreamSynchronize(kStream));
    if (agg != nullptr) download(agg, L.agg, (size_t)L.rows);
    return 0;
}

// The one body of spmv_amd_amg_stage (k = 0: single vectors on the default stream) and spmv_amd_amg_multi_stage (amg_multi.hip; k = 1..8:
// blocks of k columns, every column running)
int spmv_amd::amg_stage(const char* stage, int k, SpmvAmdAmgStageArgs* a) {
    // argument checks: all before the first HIP call
    if (stage == nullptr) return fail("stage: none named (residual_restrict, prolong_correct)"), 1;
    const bool restrict_stage = !strcmp(stage, "residual_restrict");
    if (!restrict_stage && strcmp(stage, "prolong_correct") != 0) return fail("stage: unknown (residual_restrict, prolong_correct)"), 1;
    if (a == nullptr) return fail("stage: null arguments"), 1;
    if (a->rows < 1 || a->coarse_rows < 1 || (restrict_stage && a->cols < 1)) return fail("stage: a size below 1"), 1;
    const auto aligned = [](const void* p, uintptr_t to) { return p != nullptr && ((uintptr_t)p & (to - 1)) == 0; };
    const uintptr_t block = k > 0 && k % 2 == 0 ? 16 : 8;  // a block vector: 16-byte accesses where k is even
    if (restrict_stage) {
        if (!aligned(a->row_ptr, 4) || !aligned(a->col_idx, 4) || !aligned(a->values, 8)) return fail("stage: a null or misaligned CSR array"), 1;
        if (!aligned(a->agg_ptr, 4) || !aligned(a->members, 4)) return fail("stage: a null or misaligned member list"), 1;
        if (k == 0 && (!aligned(a->z, 8) || !aligned(a->r, 8) || !aligned(a->coarse, 8)))
            return fail("stage: z, r and the coarse vector must be 8-byte aligned"), 1;
    } else if (!aligned(a->agg, 4) || (k == 0 && (!aligned(a->z, 16) || !aligned(a->coarse, 8)))) {
        return fail("stage: agg must be 4-byte, z 16-byte and the coarse vector 8-byte aligned"), 1;
    }
    if (k > 0 && (!aligned(a->z, block) || (restrict_stage && !aligned(a->r, block)) || !aligned(a->coarse, block)))
        return fail("stage: a block vector must be 8-byte aligned, 16-byte where k is even"), 1;

    // the index arrays, read back: nothing is launched on an index outside its range
    const auto ascending_from_zero = [](const std::vector<int>& p) {
        if (p[0] != 0) return false;
        for (size_t i = 1; i < p.size(); ++i)
            if (p[i] < p[i - 1]) return false;
        return true;
    };
    const auto all_within = [](const std::vector<int>& v, int bound) {
        for (const int x : v)
            if (x < 0 || x >= bound) return false;
        return true;
    };
    if (restrict_stage) {
        std::vector<int> rp((size_t)a->rows + 1), ap((size_t)a->coarse_rows + 1);
        download(rp.data(), a->row_ptr, rp.size());
        download(ap.data(), a->agg_ptr, ap.size());
        if (!ascending_from_zero(rp) || !ascending_from_zero(ap)) return fail("stage: row_ptr or agg_ptr does not ascend from 0: refused"), 1;
        std::vector<int> ci((size_t)rp.back()), mem((size_t)ap.back());
        download(ci.data(), a->col_idx, ci.size());
        download(mem.data(), a->members, mem.size());
        if (!all_within(ci, a->cols) || !all_within(mem, a->rows)) return fail("stage: a column or a member lies outside its range: refused"), 1;
        SlabCsr v;
        v.row_ptr = a->row_ptr, v.col_idx = a->col_idx, v.values = a->values;
        v.n_local = v.n_global = a->rows;
        v.nnz_local = rp.back();
        if (k == 0) launch_amg_residual_restrict(v, a->coarse_rows, a->agg_ptr, a->members, a->z, a->r, a->coarse);
        else launch_amg_residual_restrict_multi(k, v, a->coarse_rows, a->agg_ptr, a->members, nullptr, a->z, a->r, a->coarse);
    } else {
        std::vector<int> agg((size_t)a->rows);
        download(agg.data(), a->agg, agg.size());
        if (!all_within(agg, a->coarse_rows)) return fail("stage: an aggregate lies outside the coarse vector: refused"), 1;
        if (k == 0) launch_amg_prolong_correct((size_t)a->rows, a->agg, a->coarse, a->z);
        else launch_amg_prolong_correct_multi(k, (size_t)a->rows, a->agg, nullptr, a->coarse, a->z);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

extern "C" int spmv_amd_amg_stage(const char* stage, SpmvAmdAmgStageArgs* a) { return spmv_amd::amg_stage(stage, 0, a); }
#endif  // SPMV_AMD_LAB
