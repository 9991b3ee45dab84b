// cg_slab_api.hip -- the slab's accessors (cg_slab.hpp): what a slab is, what creation did, the last solve's history and timings;
// in the LAB build the options and the single stages the tests drive; time_spmv. Nothing here decides anything about a solve.
#include <limits>

#include "cg_slab.hpp"

// Which shape this slab's loop takes and who decided: "single rank" (": direction update inside the block SpMV" where
// LoopShape::fused_direction holds with detailed timers off), "pipeline", "plain: <why>". A static string.
extern "C" const char* spmv_amd_cg_slab_loop_shape(const SpmvAmdCgSlab* s) {
    if (!s->comm->exchanges_halos()) return loop_shape(s).fused_direction ? "single rank: direction update inside the block SpMV" : "single rank";
    if (!s->no_overlap) {
        if (!loop_shape(s).pipeline) return "plain: the in-place form (ring 1) or a slab too thin to split";
        return s->comm->pipeline_verdict > 0 ? "pipeline (verified against the plain order at creation)" : "pipeline";
    }
    return s->comm->pipeline_verdict < 0 ? "plain: the pipeline's residual history differed from the plain order's in the creation check"
                                         : "plain: SPMV_AMD_NO_OVERLAP=1";
}
extern "C" int spmv_amd_cg_slab_gather(SpmvAmdCgSlab* s, double* x_full) {
    const int P = s->comm->world;
    std::vector<int> counts((size_t)P), displs((size_t)P);
    for (int r = 0; r < P; ++r) spmv_amd_partition_rows(s->n, P, r, &displs[r], &counts[r]);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    if (s->comm->rank != 0)  // non-root ranks keep their own slab in place, like the reference (:831-833)
        download(x_full + s->row_offset, s->x, (size_t)s->n_local);
    WatchdogScope guard("gathering the solution on rank 0", s->comm->rank, -1, report_slab_state, s);
    s->comm->gather_to_root(s->x, s->n_local, x_full, counts.data(), displs.data());
    return 0;
}

extern "C" int spmv_amd_cg_slab_history(SpmvAmdCgSlab* s, double* out, int cap) { return copy_history(s->history, out, cap); }

extern "C" int spmv_amd_cg_slab_spmv(SpmvAmdCgSlab* s, const double* x_full, double* y_local) {
    upload(s->p, x_full + s->row_offset, (size_t)s->n_local);
    if (s->has_prev && s->row_offset >= s->halo) upload(s->p - s->halo, x_full + s->row_offset - s->halo, (size_t)s->halo);
    if (s->has_next && s->row_offset + s->n_local + s->halo <= s->n) upload(s->p + s->n_local, x_full + s->row_offset + s->n_local, (size_t)s->halo);
#ifdef SPMV_AMD_LAB
    // "first_store" 0 with the in-loop form: the block launch that leaves A x unstored on its fast blocks (y comes back as NaN there)
    const bool unstored = s->spmv_with_dot && !s->lab_first_store;
    if (unstored) HIP_CHECK(hipMemsetAsync(s->Ap, 0xFF, (size_t)s->n_local * sizeof(double), s->compute));
    slab_spmv(s, /*with_dot=*/s->spmv_with_dot, /*overlap=*/false, nullptr, nullptr, nullptr, nullptr, false, unstored);
#else
    slab_spmv(s, /*with_dot=*/s->spmv_with_dot, /*overlap=*/false, nullptr);
#endif
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(y_local, s->Ap, (size_t)s->n_local);
    return 0;
}

extern "C" void spmv_amd_cg_slab_info(const SpmvAmdCgSlab* s, int* row_offset, int* n_local, int* local_nnz) {
    if (row_offset) *row_offset = s->row_offset;
    if (n_local) *n_local = s->n_local;
    if (local_nnz) *local_nnz = (int)s->A.view.nnz_local;
}

extern "C" const char* spmv_amd_cg_slab_variant(const SpmvAmdCgSlab* s) { return s->variant_name; }
// The coefficients the slab's SpMV streams: 0 = the CSR values, 1 = the symmetric planes (kernels.hpp, SymPlanes).
extern "C" int spmv_amd_cg_slab_coefficient_form(const SpmvAmdCgSlab* s) { return s->planes_on ? 1 : 0; }

// Tile classes of a slab in the symmetric form (kernels.hpp, SymPlanes): *total = the row-lds tiles of the slab's grid rows that are
// evaluated from the planes (global grid rows 1 .. n-2), *uniform = how many of them hold the slab-wide quintuple in every
// coefficient they multiply and therefore load none. Both 0 for a slab that keeps the CSR form. Returns 0.
extern "C" int spmv_amd_cg_slab_uniform_tiles(const SpmvAmdCgSlab* s, long long* uniform, long long* total) {
    const bool have = s->planes_alloc != nullptr && s->tile_classes != nullptr;
    if (uniform) *uniform = have ? s->tiles_uniform : 0;
    if (total) *total = have ? s->tiles_total : 0;
    return 0;
}

// What placement at creation did: {0, candidates timed, SpMV ms (mean of an early and a late direction buffer as x) where the
// coefficients were, ms where they are now}. 0 values = it did not run.
extern "C" int spmv_amd_cg_slab_placement(const SpmvAmdCgSlab* s, double* out, int cap) {
    return copy_history(s->placement, out, cap);  // min(count, cap) values out, returns count
}
// Wall ms of creation's set-up phases (none of it inside any timed region): {matrix to HBM, streams + vectors, verification +
// launch plans, coefficient placement trial, tile-run trial}. Returns 5.
extern "C" int spmv_amd_cg_slab_setup_ms(const SpmvAmdCgSlab* s, double* out, int cap) {
    for (int i = 0; i < 5 && i < cap; ++i) out[i] = s->setup_ms[i];
    return 5;
}
// Row-lds tiles per XCD and run as tuned at creation: {rule, kept, SpMV ms with the rule, ms kept}. Returns 4, or 0 if the
// trial did not run (small slab, another kernel, SPMV_AMD_ROWLDS_GROUP set).
extern "C" int spmv_amd_cg_slab_tile_runs(const SpmvAmdCgSlab* s, double* out, int cap) {
    return copy_history(s->tile_runs, out, cap);
}
// The in-loop SpMV launches of the last solve one by one (ms, iteration order; only the launches that were timed: every one on
// slabs of >= 1e8 rows, every fourth below). Returns how many there are.
extern "C" int spmv_amd_cg_slab_spmv_launch_ms(const SpmvAmdCgSlab* s, float* out, int cap) {
    const int count = (int)s->last_spmv_each.size();
    for (int i = 0; i < count && i < cap; ++i) out[i] = s->last_spmv_each[i];
    return count;
}
extern "C" void spmv_amd_cg_slab_set_timeline(SpmvAmdCgSlab* s, int on) { s->timeline_on = on != 0; }

#ifdef SPMV_AMD_LAB
// (LAB build only; every entry point from here to the #endif is described in include/spmv_amd/lab.h.) Options of an existing
// slab, for A/B measurements on the SAME allocations. Returns 0, or -1 for an unknown name or value.
extern "C" int spmv_amd_cg_slab_set_option(SpmvAmdCgSlab* s, const char* name, long long value) {
    if (strcmp(name, "late_bulk") == 0) s->late_bulk = value != 0, s->late_predict = value == 2;  // 1: the protocol in every iteration, 2: where convergence is near (the default rule)
    else if (strcmp(name, "lead_rows") == 0) s->lead_rows = value < (long long)kUnit ? kUnit : round_down((size_t)value);
    else if (strcmp(name, "run_ahead") == 0) s->run_ahead = value != 0, s->guess_far_always = value == 2;
    else if (strcmp(name, "no_overlap") == 0) s->no_overlap = value != 0 || s->comm->pipeline_verdict < 0;  // a refused pipeline stays refused
    else if (strcmp(name, "stop_at") == 0) s->stop_at = value > 0 ? (int)value : 0;
    else if (strcmp(name, "spmv_event_stride") == 0) s->spmv_event_stride = (int)value;
    else if (strcmp(name, "csr_coefficients") == 0) s->planes_on = value == 0 && s->planes_alloc != nullptr;  // 1: the CSR form
    else if (strcmp(name, "stream_coefficients") == 0) {  // 1: the planes on every tile, the class map ignored
        s->stream_everywhere = value != 0;
        if (s->planes_alloc != nullptr) s->planes = plane_view(s, s->planes_alloc);
    }
    else if (strcmp(name, "block_rows") == 0) {  // grid rows per block tile of the in-loop SpMV: 0 (the one-row kernel), 4 or 8
        if (value != 0 && value != 4 && value != 8) return -1;
        s->shape.knobs.rowlds_block_rows = (int)value;
        for (Stencil5Plan* p : {&s->plan_whole, &s->plan_interior, &s->plan_head, &s->plan_tail})
            if (p->variant == Stencil5Variant::RowLds) p->block_rows = (int)value;
        build_block_maps(s);
    }
    else if (strcmp(name, "fused_direction") == 0) {  // 0: the direction update as a launch of its own, 1: inside the block SpMV where eligible, 2: ... whatever the slow blocks' share
        if (value < 0 || value > 2) return -1;
        s->fused_direction = (int)value;
    }
    else if (strcmp(name, "zero_start_parts") == 0) s->zero_start_parts = (int)value & 15;  // which parts "zero_start" 1 switches on: 1 | 2 | 4 | 8 (the field says which is which)
    else if (strcmp(name, "ap_recompute") == 0) s->ap_recompute = value != 0 ? 1 : 0;  // 1: A p' recomputed by the r update where the slab is eligible (LoopShape::ap_recomputed)
    else if (strcmp(name, "first_recompute") == 0) s->first_recompute = value != 0 ? 1 : 0;  // 1: iteration 0 in the store-less form too where ap_recomputed holds (LoopShape::first_recomputed)
    else if (strcmp(name, "first_store") == 0) s->lab_first_store = value != 0;  // 0: spmv_amd_cg_slab_first_stage, and spmv() in its in-loop form, run the launch that does not store A x
    else if (strcmp(name, "direction_store") == 0) s->lab_direction_store = value != 0;  // 0: spmv_amd_cg_slab_direction_spmv runs the fused launch that does not store A p'
    else if (strcmp(name, "zero_start") == 0) s->zero_start = value != 0;  // 0: x0 always loaded, r0 stored twice (the launches of before)
    else if (strcmp(name, "spmv_with_dot") == 0) s->spmv_with_dot = value != 0;  // spmv() in its in-loop form: p.Ap partials and their sum too
    else return -1;
    return 0;
}

// The block map of a launch range as the in-loop SpMV reads it: which = 0 the whole slab, 1 the rows that need no halo.
extern "C" long long spmv_amd_cg_slab_block_map(const SpmvAmdCgSlab* s, int which, unsigned char* out, long long cap) {
    const Stencil5Plan& p = which == 0 ? s->plan_whole : s->plan_interior;
    if (p.block_map == nullptr) return 0;
    const long long count = rowlds_block_tiles(p);
    if (out != nullptr && cap > 0) HIP_CHECK(hipMemcpy(out, p.block_map, (size_t)std::min(count, cap), hipMemcpyDeviceToHost));
    return count;
}

// The slow blocks of a launch range: the indices of the block tiles whose map byte is 0, ascending.
extern "C" long long spmv_amd_cg_slab_slow_blocks(const SpmvAmdCgSlab* s, int which, int* out, long long cap) {
    const int* list = which == 0 ? s->slow_list_whole : s->slow_list_interior;
    const long long count = which == 0 ? s->slow_count_whole : s->slow_count_interior;
    if (count <= 0) return count;
    if (out != nullptr && cap > 0) HIP_CHECK(hipMemcpy(out, list, (size_t)std::min(count, cap) * sizeof(int), hipMemcpyDeviceToHost));
    return count;
}

// What the last spmv_amd_cg_slab_spmv in its in-loop form ("spmv_with_dot" 1) left beside y: the reduced sum and the partials.
extern "C" int spmv_amd_cg_slab_spmv_dot(const SpmvAmdCgSlab* s, double* pAp, double* partials, int cap) {
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipMemcpy(pAp, &s->d_s->pAp, sizeof(double), hipMemcpyDeviceToHost));
    const int count = s->plan_whole.partials;
    if (partials != nullptr && cap > 0) HIP_CHECK(hipMemcpy(partials, s->partials_spmv, (size_t)std::min(count, cap) * sizeof(double), hipMemcpyDeviceToHost));
    return count;
}

// The direction update inside the block SpMV, once, on the caller's vectors: the fused launch, the launch over the slow blocks and
// the reduction, as an iteration >= 1 of the fused loop shape enqueues them, with s->beta = beta. p_out, Ap, the partials and *pAp
// are filled with NaN beforehand. Returns the partial count, or -1 where the slab cannot take the launch.
extern "C" int spmv_amd_cg_slab_direction_spmv(SpmvAmdCgSlab* s, const double* r, const double* p_in, double beta, int iteration_matches,
                                               int converged, double* p_out, double* Ap, double* pAp, double* partials, int cap) {
    if (s->ring.size() < 2 || s->comm->exchanges_halos() || !direction_spmv_available(shape_inputs(s, false), /*cap=*/false)) return -1;
    const size_t nl = (size_t)s->n_local;
    const int iteration = 3;
    CgScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.beta = beta;
    sc.iterations = iteration;
    sc.converged = converged != 0 ? 1 : 0;
    sc.pAp = std::numeric_limits<double>::quiet_NaN();
    HIP_CHECK(hipMemcpy(s->d_s, &sc, sizeof sc, hipMemcpyHostToDevice));
    upload(s->r, r, nl);
    upload(s->ring[0], p_in, nl);
    HIP_CHECK(hipMemsetAsync(s->ring[1], 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->Ap, 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->partials_spmv, 0xFF, (size_t)s->plan_whole.partials * sizeof(double), s->compute));
    s->shape.reverse = false;
    s->reduce_mailbox = nullptr;
    const int used = slab_direction_spmv(s, s->ring[0], s->ring[1], iteration_matches != 0 ? iteration : iteration + 1, nullptr, !s->lab_direction_store);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(p_out, s->ring[1], nl);
    download(Ap, s->Ap, nl);
    if (partials != nullptr && cap > 0) download(partials, s->partials_spmv, (size_t)std::min(used, cap));
    HIP_CHECK(hipMemcpy(&sc, s->d_s, sizeof sc, hipMemcpyDeviceToHost));
    *pAp = sc.pAp;
    s->p = s->ring[0];
    return used;
}

// The r update of an iteration >= 1, once, on the caller's vectors and scalars: recompute == 0, cg_update_r_kernel on (r, Ap);
// recompute != 0, the launch of LoopShape::ap_recomputed on (r, p_new, Ap) -- Ap is read on the slow row blocks only. r_out and the
// partials (filled with NaN beforehand) come back; returns the partial count, or -1 where recompute is asked of a slab that is not
// eligible (spmv_amd_cg_slab_ap_form bit 2).
extern "C" int spmv_amd_cg_slab_update_r_stage(SpmvAmdCgSlab* s, int recompute, int reverse, const double* r, const double* p_new, const double* Ap,
                                               double rr_old, double pAp, int converged, double* r_out, double* partials, int cap) {
    if (recompute != 0 && (s->ring.size() < 2 || !s->skew_eligible || s->sym() == nullptr)) return -1;
    const size_t nl = (size_t)s->n_local;
    CgScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.rr_old = rr_old, sc.pAp = pAp, sc.converged = converged != 0 ? 1 : 0;
    HIP_CHECK(hipMemcpy(s->d_s, &sc, sizeof sc, hipMemcpyHostToDevice));
    upload(s->r, r, nl);
    upload(s->Ap, Ap, nl);
    if (recompute != 0) upload(s->ring[1], p_new, nl);
    const int count = cg_partial_count(nl);
    HIP_CHECK(hipMemsetAsync(s->partials_blas, 0xFF, (size_t)count * sizeof(double), s->compute));
    if (recompute != 0) slab_update_r_recompute(s, s->ring[1], reverse != 0);
    else launch_cg_update_r(nl, s->d_s, s->Ap, s->r, s->partials_blas, s->compute, reverse != 0);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(r_out, s->r, nl);
    if (partials != nullptr && cap > 0) download(partials, s->partials_blas, (size_t)std::min(count, cap));
    return count;
}

// The r update that recomputes A p': bit 0 = a solve would take the form now (LoopShape::ap_recomputed), bit 1 = the last solve took
// it, bit 2 = the slab's whole-slab block map is eligible (every row block all-fast or all-slow). *launches (may be null): the
// recomputing launches the last solve enqueued. s == NULL: the workspace slab of cg_solve_device (-1: there is none).
extern "C" int spmv_amd_cg_slab_ap_form(const SpmvAmdCgSlab* s, int* launches) {
    if (s == nullptr) s = cg_workspace_slab();
    if (s == nullptr) return -1;
    if (launches != nullptr) *launches = s->last_recompute_launches;
    return (loop_shape(s).ap_recomputed ? 1 : 0) | (s->last_ap_recomputed ? 2 : 0) | (s->skew_eligible ? 4 : 0);
}

// Iteration 0's r update where r0 and p0 are one vector `src` (b, or ring slot 0), once, on the caller's vectors and scalars:
// recompute == 0, cg_update_r_from_kernel on (Ap, src); recompute != 0, the out-of-place instance of LoopShape::first_recomputed on
// (src, Ap) -- Ap is read on the slow row blocks only. r_out and the partials are filled with NaN beforehand; src_back: `src` as it
// lies on the device behind the launch. Returns the partial count, or -1 where recompute is asked of a slab that is not eligible.
extern "C" int spmv_amd_cg_slab_update_r_from_stage(SpmvAmdCgSlab* s, int recompute, int reverse, const double* src, const double* Ap, double rr_old,
                                                    double pAp, int converged, double* r_out, double* src_back, double* partials, int cap) {
    if (s->ring.size() < 2 || (recompute != 0 && (!s->skew_eligible || s->sym() == nullptr))) return -1;
    const size_t nl = (size_t)s->n_local;
    CgScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.rr_old = rr_old, sc.pAp = pAp, sc.converged = converged != 0 ? 1 : 0;
    HIP_CHECK(hipMemcpy(s->d_s, &sc, sizeof sc, hipMemcpyHostToDevice));
    upload(s->ring[1], src, nl);
    upload(s->Ap, Ap, nl);
    const int count = cg_partial_count(nl);
    HIP_CHECK(hipMemsetAsync(s->r, 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->partials_blas, 0xFF, (size_t)count * sizeof(double), s->compute));
    if (recompute != 0) slab_update_r_recompute(s, s->ring[1], reverse != 0, /*r_is_p=*/true);
    else launch_cg_update_r_from(nl, s->d_s, s->Ap, s->ring[1], s->r, s->partials_blas, s->compute, reverse != 0);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(r_out, s->r, nl);
    if (src_back != nullptr) download(src_back, s->ring[1], nl);
    if (partials != nullptr && cap > 0) download(partials, s->partials_blas, (size_t)std::min(count, cap));
    return count;
}

// Iteration 0's form (slab_decisions.hpp, FirstForm: 0 stored, 1 from b, 2 from ring slot 0, 3 in place) that a solve of at least one
// iteration would take now; *last (may be null): what the last solve took.
extern "C" int spmv_amd_cg_slab_first_recompute_form(const SpmvAmdCgSlab* s, int* last) {
    if (last != nullptr) *last = s->last_first_form;
    return (int)first_form(loop_shape(s), 1);
}

// The initial stage of a solve -- the first SpMV's launch and the reduction of its partials -- once, on the slab's stored b and x0,
// in the form a solve would take now. Returns the form: bit 0 = LoopShape::zero_start, bit 1 = LoopShape::r0_in_ring; r0 == NULL:
// only that, nothing is launched. -1: a slab with neighbours or one whose first SpMV does not write the residual.
extern "C" int spmv_amd_cg_slab_initial_stage(SpmvAmdCgSlab* s, double* r0, double* r_vec, double* partials, int cap, int* count, double* rr) {
    const LoopShape L = loop_shape(s);
    const int form = (L.zero_start ? 1 : 0) | (L.r0_in_ring ? 2 : 0);
    if (r0 == nullptr) return form;
    if (L.multi || !s->fuse_init_residual) return -1;
    const size_t nl = (size_t)s->n_local;
    HIP_CHECK(hipMemsetAsync(s->d_s, 0, sizeof(CgScalars), s->compute));
    HIP_CHECK(hipMemsetAsync(s->r, 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->ring[0], 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->partials_spmv, 0xFF, (size_t)s->partials_cap * sizeof(double), s->compute));
    s->shape.reverse = false;
    s->reduce_mailbox = nullptr;
    const int used = slab_initial_residual(s, L, /*halo_in_flight=*/false);
    reduce_spmv_partials(s, used, &s->d_s->rr_new, nullptr, nullptr, 0, nullptr);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(r0, L.r0_in_ring ? s->ring[0] : s->r, nl);
    if (r_vec != nullptr) download(r_vec, s->r, nl);
    if (partials != nullptr && cap > 0) download(partials, s->partials_spmv, (size_t)std::min(used, cap));
    if (count != nullptr) *count = used;
    HIP_CHECK(hipMemcpy(rr, &s->d_s->rr_new, sizeof(double), hipMemcpyDeviceToHost));
    s->p = s->ring[0];
    return form;
}

// The first stage of a solve in the shape LoopShape::b_is_p0 -- iteration 0's block SpMV on the stored b with both partial arrays,
// the reduction of the b.b partials, the scalars' initialisation and the reduction of the b.Ab partials -- once, as a solve of at
// least one iteration enqueues them. Returns 1 where a solve would take that shape now, else 0; Ap == NULL, or 0: only that, nothing
// is launched. Ap and both partial arrays are filled with NaN beforehand.
extern "C" int spmv_amd_cg_slab_first_stage(SpmvAmdCgSlab* s, int reverse, double* Ap, double* pAp_partials, double* bb_partials, int cap, int* count,
                                            double* rr, double* pAp) {
    if (!loop_shape(s).b_is_p0) return 0;
    if (Ap == nullptr) return 1;
    const size_t nl = (size_t)s->n_local, slots = (size_t)s->plan_whole.partials;
    HIP_CHECK(hipMemsetAsync(s->d_s, 0, sizeof(CgScalars), s->compute));
    HIP_CHECK(hipMemsetAsync(s->Ap, 0xFF, nl * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->partials_spmv, 0xFF, slots * sizeof(double), s->compute));
    HIP_CHECK(hipMemsetAsync(s->partials_first, 0xFF, slots * sizeof(double), s->compute));
    s->reduce_mailbox = nullptr;
    const int used = slab_first_spmv(s, reverse != 0, nullptr, !s->lab_first_store);
    reduce_spmv_partials(s, used, &s->d_s->rr_new, nullptr, nullptr, 0, nullptr, s->partials_first);
    launch_cg_scalars_init(s->d_s, nullptr, s->compute);
    reduce_spmv_partials(s, used, &s->d_s->pAp, &s->d_s->converged, nullptr, 0, nullptr);
    HIP_CHECK(hipStreamSynchronize(s->compute));
    HIP_CHECK(hipGetLastError());
    download(Ap, s->Ap, nl);
    const size_t out = std::min(slots, (size_t)(cap > 0 ? cap : 0));
    if (pAp_partials != nullptr && out > 0) download(pAp_partials, s->partials_spmv, out);
    if (bb_partials != nullptr && out > 0) download(bb_partials, s->partials_first, out);
    if (count != nullptr) *count = used;
    CgScalars sc;
    HIP_CHECK(hipMemcpy(&sc, s->d_s, sizeof sc, hipMemcpyDeviceToHost));
    *rr = sc.rr_old, *pAp = sc.pAp;
    return 1;
}

// The stored right-hand side as it lies on the device now (n_local doubles): no solve may change a bit of it.
extern "C" int spmv_amd_cg_slab_stored_b(SpmvAmdCgSlab* s, double* b_local) {
    HIP_CHECK(hipStreamSynchronize(s->compute));
    download(b_local, s->b, (size_t)s->n_local);
    return 0;
}

// The tile class map as creation wrote it: one byte per row-lds tile, 1 = uniform.
extern "C" long long spmv_amd_cg_slab_tile_classes(const SpmvAmdCgSlab* s, unsigned char* out, long long cap) {
    if (s->tile_classes == nullptr) return 0;
    const long long count = (long long)s->tile_class_count;
    if (out != nullptr && cap > 0) HIP_CHECK(hipMemcpy(out, s->tile_classes, (size_t)std::min(count, cap), hipMemcpyDeviceToHost));
    return count;
}
#endif  // SPMV_AMD_LAB
extern "C" const char* spmv_amd_cg_slab_timeline_names(void) { return kTimelineNames; }
extern "C" int spmv_amd_cg_slab_timeline(const SpmvAmdCgSlab* s, double* out, int cap) {
    return copy_history(s->timeline_us, out, cap);
}

extern "C" int spmv_amd_cg_slab_time_spmv(SpmvAmdCgSlab* s, int reps, float* ms_each) {
    HIP_CHECK(hipMemsetAsync(&s->d_s->converged, 0, sizeof(int), s->compute));
    EventTimer t;
    // a slab whose loop takes the direction update inside the block SpMV: that launch (+ the one over the slow blocks) is its SpMV stage
    const bool fused = loop_shape(s).fused_direction;
    if (fused) {
        CgScalars sc;
        memset(&sc, 0, sizeof sc);
        sc.beta = 0.5, sc.iterations = 1;
        HIP_CHECK(hipMemcpyAsync(s->d_s, &sc, sizeof sc, hipMemcpyHostToDevice, s->compute));
        HIP_CHECK(hipStreamSynchronize(s->compute));
    }
    for (int i = 0; i < reps; ++i) {
        t.begin(s->compute);
        if (fused) {
            const DirectionSpmv d{s->d_s, 1, s->device_form, s->r, s->ring[0], s->ring[1], s->slow_list_whole, s->slow_count_whole};
            (void)launch_stencil5_direction_spmv(s->A.view, s->plan_whole, d, s->Ap, 1.0, s->partials_spmv, false, s->compute, *s->sym());
        } else {
            (void)launch_stencil5_spmv(s->A.view, s->plan_whole, s->p, s->Ap, 1.0, s->fused_dot ? s->partials_spmv : nullptr,
                                       nullptr, false, s->compute, nullptr, s->sym());
        }
        t.end(s->compute);
        ms_each[i] = t.elapsed_ms();
    }
    HIP_CHECK(hipGetLastError());
    return 0;
}
