// cg_slab_create.hip -- creation and destruction of a slab (cg_slab.hpp): streams, the vector arena and the direction ring, the
// symmetric planes, tile classes and block maps, the launch plans, the placement and tile-run trials, and the creation check of the
// overlapped pipeline. The arithmetic of the layouts and the ring's length is slab_decisions.hpp's; here it is allocated and timed.
#include "cg_slab.hpp"

namespace spmv_amd {
namespace slab {

// (Re)binds a borrowed-operator slab to `op`: asks for the operator's fused launch and sizes the partial buffer for it.
// Called at creation and at the start of every cg_solve_device (the operator may have been re-initialised in between).
void adopt_operator(SpmvAmdCgSlab* s, SpmvOperator* op) {
    s->op = op;
    s->fused = fused_spmv_of(op);
    s->fused_dot = s->fused.partials > 0;
    s->fuse_init_residual = s->fused_dot && s->fused.can_init;
    s->variant_name = s->fused_dot ? "operator/fused-launch" : "operator/run_device+dot";
    if (s->fused.partials > s->partials_cap) {
        device_release(s->partials_spmv);
        s->partials_cap = s->fused.partials;
        s->partials_spmv = device_alloc<double>((size_t)s->partials_cap);
        HIP_CHECK(hipMemset(s->partials_spmv, 0, (size_t)s->partials_cap * sizeof(double)));
    }
}

static void place_coefficients(SpmvAmdCgSlab* s);  // below
static void tune_tile_runs(SpmvAmdCgSlab* s);

SymPlanes plane_view(const SpmvAmdCgSlab* s, const double* base) {
    SymPlanes v;
    v.ce = base;
    v.s = base + s->planes_s_offset;
    v.cls = s->stream_everywhere ? nullptr : s->tile_classes;
    v.w = s->quintuple[0], v.c = s->quintuple[1], v.e = s->quintuple[2], v.n = s->quintuple[3], v.s5 = s->quintuple[4];
    return v;
}

// One device counter of type T: zeroed, handed to `launch` (a check that writes it), read back behind it on `q`, freed.
template <class T, class Launch>
static T device_check(hipStream_t q, Launch&& launch) {
    T* d = device_alloc<T>(1);
    HIP_CHECK(hipMemsetAsync(d, 0, sizeof(T), q));
    launch(d);
    T h{};
    HIP_CHECK(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, q));
    HIP_CHECK(hipStreamSynchronize(q));
    device_release(d);
    return h;
}

// The tile class map of a slab that keeps the planes. The quintuple is the CSR row of one fully interior grid point near the
// slab's middle: a bad pick costs speed, never correctness -- every tile is compared against it. A slab without a grid row that is
// evaluated from the planes (or a grid of fewer than three columns) has no map.
static void classify_tiles(SpmvAmdCgSlab* s) {
    const int n = s->grid;
    const int gfirst = s->row_offset / n, rows = s->n_local / n;
    const int lo = std::max(gfirst, 1), hi = std::min(gfirst + rows, n - 1);  // global grid rows [lo, hi) take the planes
    if (hi <= lo || n < 3) return;
    const int col_tiles = rowlds_col_tiles(n);
    s->tiles_total = (long long)(hi - lo) * col_tiles;
    const long long lr = (long long)(lo + (hi - lo) / 2 - gfirst) * n + n / 2;
    int first = 0;
    HIP_CHECK(hipMemcpy(&first, s->A.view.row_ptr + lr, sizeof(int), hipMemcpyDeviceToHost));
    double row[5];  // [N, W, C, E, S]
    HIP_CHECK(hipMemcpy(row, s->A.view.values + first, sizeof(row), hipMemcpyDeviceToHost));
    const double q[5] = {row[1], row[2], row[3], row[0], row[4]};
    memcpy(s->quintuple, q, sizeof(q));
    s->tile_class_count = (size_t)rows * col_tiles;
    const size_t bytes = s->tile_class_count;
    s->tile_classes = device_try_alloc<unsigned char>(bytes);
    if (s->tile_classes == nullptr) {
        s->tile_class_count = 0;
        return;
    }
    HIP_CHECK(hipMemsetAsync(s->tile_classes, 0, bytes, s->compute));
    s->tiles_uniform = (long long)device_check<unsigned long long>(
        s->compute, [&](unsigned long long* d_count) { launch_classify_tiles(s->A.view, q, s->tile_classes, d_count, s->compute); });
}

// Points the whole-slab and interior plans at their block maps (plans are re-made when the tile runs are tuned).
static void attach_block_maps(SpmvAmdCgSlab* s) {
    s->plan_whole.block_map = s->block_map_whole;
    s->plan_interior.block_map = s->block_map_interior;
}

// The block maps of the two launch ranges the in-loop SpMV takes, from the class map, for the plans' block_rows. A slab without a
// class map, or with block_rows 0, has none: its launches are the one-row kernel's.
void build_block_maps(SpmvAmdCgSlab* s) {
    HIP_CHECK(hipStreamSynchronize(s->compute));
    device_release(s->block_map_whole);
    device_release(s->block_map_interior);
    device_release(s->slow_list_whole);
    device_release(s->slow_list_interior);
    device_release(s->row_block_fast);
    s->slow_count_whole = s->slow_count_interior = 0;
    s->skew_eligible = false;
    if (s->tile_classes != nullptr) {
        const auto map_of = [&](const Stencil5Plan& p) -> unsigned char* {
            const int blocks = rowlds_block_tiles(p);
            unsigned char* map = blocks > 0 ? device_try_alloc<unsigned char>((size_t)blocks) : nullptr;
            if (map != nullptr) launch_block_map(s->tile_classes, p, map, s->compute);
            return map;
        };
        s->block_map_whole = map_of(s->plan_whole);
        s->block_map_interior = map_of(s->plan_interior);
        HIP_CHECK(hipStreamSynchronize(s->compute));
        // the slow blocks of a range, listed once (a map is one byte per block tile: 0.8 MB at 20 000^2)
        const auto list_of = [&](const Stencil5Plan& p, const unsigned char* map, int* count) -> int* {
            *count = 0;
            if (map == nullptr) return nullptr;
            std::vector<unsigned char> h((size_t)rowlds_block_tiles(p));
            HIP_CHECK(hipMemcpy(h.data(), map, h.size(), hipMemcpyDeviceToHost));
            std::vector<int> slow;
            for (size_t b = 0; b < h.size(); ++b)
                if (h[b] == 0) slow.push_back((int)b);
            if (slow.empty()) return nullptr;
            int* list = device_try_alloc<int>(slow.size());
            if (list == nullptr) {
                *count = -1;  // no list: the range keeps the two-launch form
                return nullptr;
            }
            HIP_CHECK(hipMemcpy(list, slow.data(), slow.size() * sizeof(int), hipMemcpyHostToDevice));
            *count = (int)slow.size();
            return list;
        };
        s->slow_list_whole = list_of(s->plan_whole, s->block_map_whole, &s->slow_count_whole);
        s->slow_list_interior = list_of(s->plan_interior, s->block_map_interior, &s->slow_count_interior);
        // the whole-slab map by row block, for the r update that recomputes A p' (skew_geometry.hpp): a slab without halo rows only
        if (s->block_map_whole != nullptr && s->halo == 0 && s->plan_whole.first_row == 0 && s->plan_whole.last_row == s->n_local) {
            const Stencil5Plan& p = s->plan_whole;
            const int col_tiles = p.row_blocks, row_blocks = rowlds_block_tiles(p) / col_tiles;
            std::vector<unsigned char> map((size_t)rowlds_block_tiles(p)), fast((size_t)row_blocks);
            HIP_CHECK(hipMemcpy(map.data(), s->block_map_whole, map.size(), hipMemcpyDeviceToHost));
            const bool eligible = skew_eligible(map.data(), row_blocks, col_tiles, fast.data());
            s->row_block_fast = eligible ? device_try_alloc<unsigned char>(fast.size()) : nullptr;
            if (s->row_block_fast != nullptr) HIP_CHECK(hipMemcpy(s->row_block_fast, fast.data(), fast.size(), hipMemcpyHostToDevice));
            s->skew_eligible = s->row_block_fast != nullptr;
        }
    }
    attach_block_maps(s);
}

// Fills the reserved planes from the verified CSR and checks them bit for bit (launch_verify_sym_planes); any mismatch, an
// unverified structure or a launch that is not row-lds frees them again: the slab keeps the CSR form.
static void settle_planes(SpmvAmdCgSlab* s) {
    if (s->planes_alloc == nullptr) return;
    bool keep = s->A.view.verified_stencil && s->fuse_init_residual;  // every launch of the slab is a row-lds launch
    if (keep) {
        launch_fill_sym_planes(s->A.view, s->planes_alloc, s->planes_alloc + s->planes_s_offset, s->compute);
        s->planes = plane_view(s, s->planes_alloc);
        keep = device_check<int>(s->compute, [&](int* d_flag) { launch_verify_sym_planes(s->A.view, s->planes, d_flag, s->compute); }) == 0;
    }
    if (!keep) {
        device_release(s->planes_alloc);
        s->planes = SymPlanes{};
    } else {
        classify_tiles(s);
        s->planes = plane_view(s, s->planes_alloc);
        build_block_maps(s);
        // the fact LoopShape::b_is_p0 rests on, and the second partial array of its launch; without the array the fact is not recorded
        if (device_check<int>(s->compute, [&](int* d_bad) { launch_rows_plus_zero(s->A.view, d_bad, s->compute); }) == 0)
            s->partials_first = device_try_alloc<double>((size_t)s->plan_whole.partials);
        s->zero_rows_plus_zero = s->partials_first != nullptr;
    }
    s->planes_on = keep;
}

// Set-up phase clock: wall time since `from`, after everything enqueued so far has finished.
static double setup_phase_ms(std::chrono::steady_clock::time_point& from) {
    HIP_CHECK(hipDeviceSynchronize());
    const auto now = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(now - from).count();
    from = now;
    return ms;
}

// The four launch plans, made at creation and again when the tile runs are tuned: the whole slab, the rows that need no halo, the
// slab's first / last grid row.
static void make_plans(SpmvAmdCgSlab* s) {
    const RowRange r = s->halo_free();
    const auto plan = [&](int a, int b) { return plan_stencil5(s->A.view, a, b > a ? b : a, Stencil5Variant::Auto, s->shape); };
    s->plan_whole = plan(0, s->n_local);
    s->plan_interior = plan(r.lo, r.hi);
    s->plan_head = plan(0, r.lo);
    s->plan_tail = plan(r.hi, s->n_local);
}

void make_common(SpmvAmdCgSlab* s) {
    const size_t nl = (size_t)s->n_local;
    auto phase = std::chrono::steady_clock::now();
    const Sides sides = slab_sides(s->comm->exchanges_halos(), s->part_rank, s->part_world, s->comm->self_neighbour, s->grid);
    s->has_prev = sides.has_prev, s->has_next = sides.has_next, s->halo = sides.halo;
    s->A.view.halo_before = s->has_prev ? s->halo : 0;
    s->A.view.halo_after = s->has_next ? s->halo : 0;
    if (s->op != nullptr) {
        // borrowed operator: its run_device enqueues on the default stream (reference spmv_stencil_csr_direct.cu:267-271),
        // so the whole solve runs there; one rank, no halo exchange, no side stream
        s->compute = nullptr;
        s->side = nullptr;
        s->owns_streams = false;
    } else {
        HIP_CHECK(hipStreamCreateWithFlags(&s->compute, hipStreamNonBlocking));
        // the side stream has the DEFAULT priority: a highest-priority one slows every kernel of the compute stream
        HIP_CHECK(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
    }
    HIP_CHECK(hipEventCreateWithFlags(&s->ev_p_ready, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&s->ev_halo_done, hipEventDisableTiming));
    s->shape = current_launch_shape();
    // the local part of every halo-carrying buffer starts on a 4 KiB boundary whatever the halo length, like the plain
    // allocations of r, Ap, x; r, Ap (slots 0 and 1) and the direction buffers lie one `pitch` apart in the vector arena
    const auto [lead, slot_doubles, pitch] = slot_layout(nl, s->halo);
    s->slot_doubles = slot_doubles;
    s->slot_lead = lead;
    s->x = device_alloc<double>(nl);
    s->b = device_alloc<double>(nl);
    s->x0_alloc = device_alloc<double>(slot_doubles);
    s->x0 = s->x0_alloc + lead;
    HIP_CHECK(hipMemset(s->x0_alloc, 0, slot_doubles * sizeof(double)));
    {
        // as many direction buffers as fit comfortably (default 16, SPMV_AMD_P_RING=1 keeps the in-place update)
        const char* forced = getenv("SPMV_AMD_P_RING");
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        const size_t per_slot = pitch * sizeof(double);
        if (may_take_planes(s->op == nullptr, s->grid, s->shape.knobs.rowlds_min_grid, s->n_local, s->row_offset)) {
            // the symmetric planes before the ring (24 B per row + one grid row: 9.6 GB at 4e8 rows), where a ring of 4 still fits
            // beside them. Optional: a device that cannot provide them leaves the slab in the CSR form. Whether the slab keeps them
            // is decided once the structure is verified and the plans are made (settle_planes).
            const PlaneLayout planes = plane_layout(nl, s->grid);
            if (planes_fit(free_b, planes.total * sizeof(double), per_slot)) {
                s->planes_alloc = device_try_alloc<double>(planes.total);
                if (s->planes_alloc != nullptr) {
                    s->planes_doubles = planes.total;
                    s->planes_s_offset = planes.s_offset;
                    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
                }
            }
        }
        const int want = ring_length(forced ? atoi(forced) : kMaxRingSlots, per_slot, free_b, s->op != nullptr, kMaxRingSlots);
        s->vec_arena = device_alloc<double>((size_t)(2 + want) * pitch);
        HIP_CHECK(hipMemset(s->vec_arena, 0, (size_t)(2 + want) * pitch * sizeof(double)));
        s->r = s->vec_arena;
        s->Ap = s->vec_arena + pitch;
        s->ring_alloc.clear();
        s->ring.clear();
        for (int k = 0; k < want; ++k) {
            double* a = s->vec_arena + (size_t)(2 + k) * pitch;
            s->ring_alloc.push_back(a);
            s->ring.push_back(a + lead);
        }
        s->p_alloc = s->ring_alloc[0];
        s->p = s->ring[0];
        s->ring_slots = want;
        s->d_alpha_ring = device_alloc<double>(kMaxRingSlots);
        HIP_CHECK(hipMemset(s->d_alpha_ring, 0, kMaxRingSlots * sizeof(double)));
    }
    if (const char* v = getenv("SPMV_AMD_NO_OVERLAP")) s->no_overlap = v[0] == '1';
    if (const char* v = getenv("SPMV_AMD_FUSED_DIRECTION")) s->fused_direction = v[0] == '1' ? 1 : 0;
    if (const char* v = getenv("SPMV_AMD_ZERO_START")) s->zero_start = v[0] != '0';
    if (const char* v = getenv("SPMV_AMD_AP_RECOMPUTE")) s->ap_recompute = v[0] == '1' ? 1 : 0;
    if (const char* v = getenv("SPMV_AMD_FIRST_RECOMPUTE")) s->first_recompute = v[0] == '1' ? 1 : 0;
    {
        // grid rows per block tile: what SPMV_AMD_ROWLDS_BLOCK_ROWS asks, else by the slab's kind (the plans are made further down)
        const char* v = getenv("SPMV_AMD_ROWLDS_BLOCK_ROWS");
        s->shape.knobs.rowlds_block_rows =
            default_block_rows(v && *v ? atoi(v) : -1, s->comm->exchanges_halos(), s->op == nullptr, s->ring_slots, s->fused_direction);
    }
#ifdef SPMV_AMD_LAB
    if (const char* v = getenv("SPMV_AMD_TEST_WEDGE_OVERLAPPED_EXCHANGE")) s->test_wedge_overlapped_exchange = atoi(v);
#endif
    if (const char* v = getenv("SPMV_AMD_ROCTX")) s->roctx_always = v[0] == '1';
    s->late_bulk = late_bulk_default(nl);
    s->partials_blas = device_alloc<double>(dot_scratch_doubles(nl));
    HIP_CHECK(hipMemset(s->partials_blas, 0, dot_scratch_doubles(nl) * sizeof(double)));
    s->reduce_stage = reduce_scratch_alloc();
    s->d_halo_flag = device_alloc<unsigned>(1);
    HIP_CHECK(hipMemset(s->d_halo_flag, 0, sizeof(unsigned)));
    s->d_s = device_alloc<CgScalars>(1);
    HIP_CHECK(hipMemset(s->d_s, 0, sizeof(CgScalars)));
    HIP_CHECK(hipHostMalloc((void**)&s->h_poll, sizeof(*s->h_poll), hipHostMallocCoherent | hipHostMallocMapped));
    memset(s->h_poll, 0, sizeof(*s->h_poll));
    if (s->op != nullptr) {
        adopt_operator(s, s->op);
        launch_fill(s->b, nl, 1.0, s->compute);
        launch_fill(s->x0, nl, 0.0, s->compute);
        s->x0_known_zero = true;
        HIP_CHECK(hipDeviceSynchronize());
        return;
    }
    s->setup_ms[1] = setup_phase_ms(phase);
    s->A.verify_stencil(s->compute);
    {
        // dot partials: one slot per launched wave; the launch geometry is a fixed function of the
        // slab and the row range, so size for the larger of the two ways a SpMV is issued
        make_plans(s);
        const auto [lo, hi] = s->halo_free();
        const int whole = s->plan_whole.partials;
        const int split = (hi > lo ? s->plan_interior.partials : 0) + (lo > 0 ? s->plan_head.partials : 0) +
                          (hi < s->n_local ? s->plan_tail.partials : 0);
        s->partials_cap = whole > split ? whole : split;
        s->partials_spmv = device_alloc<double>((size_t)s->partials_cap);
        HIP_CHECK(hipMemset(s->partials_spmv, 0, (size_t)s->partials_cap * sizeof(double)));
        s->variant_name = s->plan_whole.name;
        // unverified / unaligned slabs run the row-generic kernel and use the plain dot kernel
        s->fused_dot = s->plan_whole.variant != Stencil5Variant::RowGeneric;
        // the initial residual rides in the first SpMV where every launch of the slab is a row-lds launch
        const auto rowlds = [&](const Stencil5Plan& p) { return p.last_row <= p.first_row || p.variant == Stencil5Variant::RowLds; };
        s->fuse_init_residual = s->plan_whole.variant == Stencil5Variant::RowLds && rowlds(s->plan_interior) && rowlds(s->plan_head) && rowlds(s->plan_tail);
    }
    settle_planes(s);
    s->setup_ms[2] = setup_phase_ms(phase);
    if (s->setup_trials) place_coefficients(s);
    s->setup_ms[3] = setup_phase_ms(phase);
    if (s->setup_trials) tune_tile_runs(s);
    launch_fill(s->b, nl, 1.0, s->compute);   // default right-hand side b = 1
    launch_fill(s->x0, nl, 0.0, s->compute);  // default initial guess x0 = 0
    s->x0_known_zero = true;
    s->setup_ms[4] = setup_phase_ms(phase);
}

// The coefficient stream's place. In the vector arena Ap shares its region with the first direction buffers and not
// with the later ones, so the one thing left to chance is whether the coefficients V lie in Ap's class: if they do, every iteration
// on a later buffer runs 2 % slow. So the coefficients are offered up to two MORE allocations one region apart, each timed on the
// SpMV from an early and from a late direction buffer, and the fastest is kept. Set-up work; the values are copied, never changed.
// Slabs of >= 16 Mi rows that own their matrix. Optional in every respect: a candidate the device cannot provide ends the trial
// with the array as it was, and the copy that loses is freed (DeviceCsr::separate_values).
static bool wants_coefficient_placement(size_t n_local) { return wants_coefficient_placement(n_local, placement_candidates()); }

static void place_coefficients(SpmvAmdCgSlab* s) {
    const size_t nl = (size_t)s->n_local;
    if (s->op != nullptr || !wants_coefficient_placement(nl) || s->ring.size() < 4 || s->A.values == nullptr) return;
    hipStream_t q = s->compute;
    // Every tile that is evaluated from the planes is uniform: the SpMV being timed reads no plane value, so the trial skips its
    // copies (9.6 GB each at 4e8 rows) -- the candidates are still timed and recorded, and a candidate that is kept receives the
    // planes then (class-0 paths of the A/B options read them).
    const bool nothing_streamed = s->planes_on && s->tiles_total > 0 && s->tiles_uniform == s->tiles_total && !s->stream_everywhere;
    // the coefficient stream the loop reads: the symmetric planes where the slab keeps them, else the CSR values
    const bool planes = s->planes_on;
    const size_t count = planes ? s->planes_doubles : (size_t)s->A.view.nnz_local;
    const double* early = s->ring[1];
    const double* late = s->ring[s->ring.size() - 3];
    launch_fill(s->ring[1], nl, 1.0, q);
    launch_fill(s->ring[s->ring.size() - 3], nl, 1.0, q);
    HIP_CHECK(hipMemsetAsync(&s->d_s->converged, 0, sizeof(int), q));
    EventTimer timer;
    double* const original = planes ? s->planes_alloc : s->A.values;
    const auto point_at = [&](double* values) {
        if (planes) s->planes = plane_view(s, values);
        else s->A.view.values = values;
    };
    auto cost = [&](double* values) {
        point_at(values);
        double total = 0.0;
        for (const double* x : {early, late}) {
            float ms[3];
            for (int i = 0; i < 4; ++i) {
                timer.begin(q);
                (void)launch_stencil5_spmv(s->A.view, s->plan_whole, x, s->Ap, 1.0, s->fused_dot ? s->partials_spmv : nullptr, nullptr, false, q,
                                           nullptr, s->sym());
                timer.end(q);
                const float t = timer.elapsed_ms();
                if (i > 0) ms[i - 1] = t;
            }
            std::sort(ms, ms + 3);
            total += ms[1];
        }
        point_at(original);
        return 0.5 * total;
    };
    int tried = 0;
    double before = 0.0, after = 0.0;
    double* best = device_alloc_best_of<double>(count, 0, [&](double* cand) {
        if (cand != original && !nothing_streamed) HIP_CHECK(hipMemcpyAsync(cand, original, count * sizeof(double), hipMemcpyDeviceToDevice, q));
        const double ms = cost(cand);
        if (cand == original) before = ms;
        return ms;
    }, &tried, nullptr, original, /*release_first=*/false);
    after = best == original ? before : cost(best);
    HIP_CHECK(hipStreamSynchronize(q));
    const bool moved = best != original && after < 0.99 * before;
    if (moved && nothing_streamed) {
        HIP_CHECK(hipMemcpyAsync(best, original, count * sizeof(double), hipMemcpyDeviceToDevice, q));
        HIP_CHECK(hipStreamSynchronize(q));
    }
    if (best != original) {
        if (!moved) device_release(best);
        else if (planes) device_release(s->planes_alloc), s->planes_alloc = best;
        else s->A.replace_values(best);  // frees `original` when it is an allocation of its own
    }
    s->A.view.values = s->A.values;
    if (planes) s->planes = plane_view(s, s->planes_alloc);
    for (double* a : s->ring_alloc) HIP_CHECK(hipMemsetAsync(a, 0, s->slot_doubles * sizeof(double), q));
    HIP_CHECK(hipStreamSynchronize(q));
    s->placement = {0.0, (double)tried, before, moved ? after : before};
}

// Row-lds tiles per XCD and run, by measurement on the slab's own vectors (device_runtime.hpp, tune_rowlds_xcd_run): the four
// launch plans are then re-made with the run length kept. Their partial counts do not depend on it.
static void tune_tile_runs(SpmvAmdCgSlab* s) {
    if (s->op != nullptr || s->ring.size() < 2) return;
    const size_t nl = (size_t)s->n_local;
    hipStream_t q = s->compute;
    double* x = s->ring[1];
    launch_fill(x, nl, 1.0, q);
    HIP_CHECK(hipMemsetAsync(&s->d_s->converged, 0, sizeof(int), q));
    double rec[4] = {0, 0, 0, 0};
    const int run = tune_rowlds_xcd_run(s->A.view, s->shape, x, s->Ap, s->fused_dot ? s->partials_spmv : nullptr, q, rec, s->sym(),
                                        s->plan_whole.block_map);
    HIP_CHECK(hipMemsetAsync(s->ring_alloc[1], 0, s->slot_doubles * sizeof(double), q));
    HIP_CHECK(hipStreamSynchronize(q));
    if (run <= 0) return;
    s->shape.knobs.rowlds_group = run;
    make_plans(s);
    attach_block_maps(s);  // the maps do not depend on the run length
    s->tile_runs.assign(rec, rec + 4);
}

static bool partition_ok(const SpmvAmdComm* comm, int grid, int n_local) {
    const Partition verdict = partition_check(comm->exchanges_halos(), grid, n_local);
    if (verdict == Partition::NeedsStencil) fprintf(stderr, "[cg-slab] multi-GPU solve needs a stencil matrix (grid_size > 0)\n");
    if (verdict == Partition::ThinnerThanGridRow) fprintf(stderr, "[cg-slab] slab of %d rows is thinner than one grid row (%d)\n", n_local, grid);
    return verdict == Partition::Ok;
}

// Every halo row of every halo-carrying buffer (x0's, the direction ring's) set to NaN (all bits one). A correct loop receives
// each of them before it reads it. Repeated solves of one system write the SAME values into the same slots every time: rows
// that were lost, or read before they arrived, would otherwise be indistinguishable from rows that travelled.
void poison_halos(SpmvAmdCgSlab* s) {
    if (s->halo == 0 || s->op != nullptr) return;
    const size_t bytes = (size_t)s->halo * sizeof(double);
    auto both_sides = [&](double* local) {
        if (s->has_prev) HIP_CHECK(hipMemsetAsync(local - s->halo, 0xFF, bytes, s->compute));
        if (s->has_next) HIP_CHECK(hipMemsetAsync(local + s->n_local, 0xFF, bytes, s->compute));
    };
    both_sides(s->x0);
    for (double* local : s->ring) both_sides(local);
}

// The pipeline hands rows between its two streams through device flags and reads the received halo rows inside a running kernel --
// constructions that cannot be proven between devices on a one-GPU box. So the FIRST slab created on a communicator that exchanges
// halos checks them where it runs: four iterations in the plain order, four in the pipeline; the two shapes give the
// same bits by construction, so any difference in the residual history on any rank -- lost or stale halo rows (the halos are set to
// NaN before each solve), a flag that never comes (the waits give up after 2 s here) -- refuses the pipeline for every slab on that
// communicator: they run the plain order, say so on stderr and in spmv_amd_cg_slab_loop_shape(). Once per communicator, outside every timed region.
static void verify_pipeline(SpmvAmdCgSlab* s) {
    SpmvAmdComm* comm = s->comm;
    if (s->op != nullptr || !comm->exchanges_halos()) return;
    if (s->no_overlap) return;  // the caller asked for the plain order: nothing to verify, nothing recorded
    const CGConfigMultiGPU few = {4, 0.0, 0, 0};
    // Whether THIS rank's slab takes the pipeline is a local fact (an odd row count, a thin last slab, the in-place form make it
    // plain) while the check is collective: every rank of the communicator runs the two solves -- a plain-shaped rank solves
    // the plain order twice -- and the verdict counts only if at least one rank really ran the pipeline.
    const bool mine = loop_shape(s).pipeline;
    if (comm->world == 1 && !mine) return;
    if (comm->pipeline_verdict == 0) {
        CGStatsMultiGPU st;
        s->selfcheck = true, s->selfcheck_late = false, s->wait_limit_s = 2.0;
        s->no_overlap = true;
        poison_halos(s);
        spmv_amd_cg_slab_solve(s, &few, &st);
        const std::vector<double> plain = s->history;
        s->no_overlap = false;
        poison_halos(s);  // what the plain solve left in the halos is exactly what the pipeline should receive: wipe it
        spmv_amd_cg_slab_solve(s, &few, &st);
        poison_halos(s);
        HIP_CHECK(hipStreamSynchronize(s->compute));
        if (s->side) HIP_CHECK(hipStreamSynchronize(s->side));
        // everything the check enqueued has run: a wait that gave up in an iteration the host had already enqueued ahead may have
        // raised the flag again after read_status cleared it
        __atomic_store_n(&s->h_poll->halo_late, 0, __ATOMIC_RELEASE);
        bool finite = true;  // NaN from a poisoned halo in the PLAIN order: the transport itself does not deliver the rows
        for (double v : plain) finite = finite && std::isfinite(v);
        if (!finite)
            fprintf(stderr, "[cg-slab] rank %d: the plain order's residual history is not finite in the creation check: the communicator's halo "
                            "exchange does not deliver this rank's neighbour rows (transport: %s)\n", comm->rank, comm->transport());
        const bool same = finite && !s->selfcheck_late && plain.size() == s->history.size() && plain.size() == 5 &&
                          memcmp(plain.data(), s->history.data(), plain.size() * sizeof(double)) == 0;
        s->selfcheck = false, s->selfcheck_late = false, s->wait_limit_s = 0.0;
        double votes[2] = {same ? 0.0 : 1.0, mine ? 1.0 : 0.0};  // {ranks whose histories differ, ranks that ran the pipeline}
        if (!same)
            fprintf(stderr, "[cg-slab] rank %d: the overlapped pipeline did NOT reproduce the plain order's residual history in the creation check\n", comm->rank);
        if (comm->world > 1) {  // every rank learns what every rank found
            double* d = device_alloc<double>(2);
            upload(d, votes, 2);
            WatchdogScope guard("creation check: all-reduce of the ranks' verdicts", comm->rank, -1, report_slab_state, s);
            comm->allreduce_sum(d, 2, s->compute);
            HIP_CHECK(hipStreamSynchronize(s->compute));
            download(votes, d, 2);
            device_release(d);
        }
        // no rank ran the pipeline (every slab thin or in place): nothing was verified, a later slab on this communicator checks again
        if (votes[0] != 0.0 || votes[1] != 0.0) comm->pipeline_verdict = votes[0] == 0.0 ? 1 : -1;
        if (comm->pipeline_verdict < 0 && comm->rank == 0)
            fprintf(stderr, "[cg-slab] %g rank(s) refused the overlapped pipeline: every solve on this communicator runs the plain order "
                            "(halo exchange on the compute stream, the reference's own)\n", votes[0]);
    }
    if (comm->pipeline_verdict < 0) s->no_overlap = true;
}

// What the creators share: the record of slab `part_rank` of `part_world`, its matrix brought to HBM by `matrix_to_hbm`, the rest.
template <class ToHbm>
static SpmvAmdCgSlab* create_slab(SpmvAmdComm* comm, int part_rank, int part_world, int n, int grid, int row_offset, int n_local, bool setup_trials,
                                  ToHbm&& matrix_to_hbm) {
    SpmvAmdCgSlab* s = new SpmvAmdCgSlab();
    s->comm = comm;
    s->part_rank = part_rank;
    s->part_world = part_world;
    s->n = n;
    s->grid = grid;
    s->row_offset = row_offset;
    s->n_local = n_local;
    s->setup_trials = setup_trials;
    s->A.separate_values = setup_trials && wants_coefficient_placement((size_t)n_local);  // the copy that loses the placement trial can then be freed
    auto phase = std::chrono::steady_clock::now();
    matrix_to_hbm(s->A);
    s->setup_ms[0] = setup_phase_ms(phase);
    make_common(s);
    verify_pipeline(s);
    return s;
}

SpmvAmdCgSlab* create_from_matrix(MatrixData* mat, SpmvAmdComm* comm, bool setup_trials) {
    if (comm == nullptr) comm = self_comm();
    if (mat->rows != mat->cols) {
        fprintf(stderr, "[cg-slab] CG needs a square matrix\n");
        return nullptr;
    }
    int row_offset = 0, n_local = 0;
    spmv_amd_partition_rows(mat->rows, comm->world, comm->rank, &row_offset, &n_local);
    if (!partition_ok(comm, mat->grid_size, n_local)) return nullptr;
    // every rank builds the CSR of the whole matrix, then keeps its slab (reference :303-331)
    if (build_csr_struct(mat) != EXIT_SUCCESS) return nullptr;
    return create_slab(comm, comm->rank, comm->world, mat->rows, mat->grid_size, row_offset, n_local, setup_trials,
                       [&](DeviceCsr& A) { A.upload_slab(csr_mat, row_offset, n_local, mat->grid_size); });
}

static SpmvAmdCgSlab* create_stencil5_slab(int n, int part_rank, int part_world, SpmvAmdComm* comm) {
    if (n < 2 || (long long)n * n > 0x7fffffffLL || 5LL * n * n - 4LL * n > 0x7fffffffLL) {
        fprintf(stderr, "[cg-slab] grid %d does not fit 32-bit CSR indices\n", n);
        return nullptr;
    }
    int row_offset = 0, n_local = 0;
    spmv_amd_partition_rows(n * n, part_world, part_rank, &row_offset, &n_local);
    if (!partition_ok(comm, n, n_local)) return nullptr;
    return create_slab(comm, part_rank, part_world, n * n, n, row_offset, n_local, /*setup_trials=*/true,
                       [&](DeviceCsr& A) { A.generate_stencil5(n, row_offset, n_local, 5.0, -1.0, nullptr); });
}
}  // namespace slab
}  // namespace spmv_amd

extern "C" SpmvAmdCgSlab* spmv_amd_cg_slab_create(MatrixData* mat, SpmvAmdComm* comm) { return create_from_matrix(mat, comm, true); }

extern "C" SpmvAmdCgSlab* spmv_amd_cg_slab_create_stencil5(int n, SpmvAmdComm* comm) {
    if (comm == nullptr) comm = self_comm();
    return create_stencil5_slab(n, comm->rank, comm->world, comm);
}

#ifdef SPMV_AMD_LAB
// (LAB build only; include/spmv_amd/lab.h.) Stand-in slab for measurements on one GPU: the slab rank `as_rank` of an `as_world`-GPU
// job would own, carried by a single-rank self-neighbour communicator (the slab mirrored at both cuts: a different linear system
// with the same work per iteration; tests/test_distributed.py, stand_in_system, checks the solve against the oracle).
extern "C" SpmvAmdCgSlab* spmv_amd_cg_slab_create_stencil5_as(int n, int as_rank, int as_world, SpmvAmdComm* comm) {
    if (comm == nullptr || comm->world != 1 || (as_world > 1 && !comm->self_neighbour)) {
        fprintf(stderr, "[cg-slab] a stand-in slab needs a single-rank self-neighbour communicator\n");
        return nullptr;
    }
    if (as_world < 1 || as_rank < 0 || as_rank >= as_world) return nullptr;
    return create_stencil5_slab(n, as_rank, as_world, comm);
}
#endif  // SPMV_AMD_LAB

extern "C" int spmv_amd_cg_slab_set_vectors(SpmvAmdCgSlab* s, const double* b_full,
                                            const double* x0_full) {
    if (b_full) upload(s->b, b_full + s->row_offset, (size_t)s->n_local);
    if (x0_full) {  // the caller's values, whatever they are: never looked at (NULL: x0 keeps its contents, and the flag with them)
        upload(s->x0, x0_full + s->row_offset, (size_t)s->n_local);
        s->x0_known_zero = false;
    }
    return 0;
}
extern "C" void spmv_amd_cg_slab_destroy(SpmvAmdCgSlab* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->compute);
    (void)hipStreamSynchronize(s->side);
    s->A.release();
    device_release(s->x);
    device_release(s->x0_alloc);
    device_release(s->b);
    s->x0 = nullptr;
    device_release(s->vec_arena);  // r, Ap and the direction buffers
    device_release(s->planes_alloc);
    device_release(s->tile_classes);
    device_release(s->block_map_whole);
    device_release(s->block_map_interior);
    device_release(s->slow_list_whole);
    device_release(s->slow_list_interior);
    device_release(s->row_block_fast);
    s->planes_on = false;
    s->r = s->Ap = s->p_alloc = s->p = nullptr;
    s->ring_alloc.clear();
    s->ring.clear();
    device_release(s->d_alpha_ring);
    device_release(s->partials_spmv);
    device_release(s->partials_blas);
    device_release(s->partials_first);
    device_release(s->reduce_stage);
    device_release(s->d_halo_flag);
    device_release(s->d_s);
    if (s->d_hist) (void)hipHostFree(s->d_hist);
    if (s->h_poll) (void)hipHostFree(s->h_poll);
    for (hipEvent_t e : s->spmv_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->tl_compute) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->tl_side) (void)hipEventDestroy(e);
    (void)hipEventDestroy(s->ev_p_ready);
    (void)hipEventDestroy(s->ev_halo_done);
    if (s->owns_streams) {
        (void)hipStreamDestroy(s->compute);
        (void)hipStreamDestroy(s->side);
    }
    delete s;
}
