// cg_slab_solve.hip -- one solve on a slab (cg_slab.hpp): the forms of the slab's SpMV, the waits on the status records and the
// halo exchange, the stages of an iteration (SolveRun) and spmv_amd_cg_slab_solve. What is decided here is decided by
// slab_decisions.hpp; this file waits, launches and prints.
#include <thread>

#include "cg_slab.hpp"

namespace spmv_amd {
namespace slab {

static double halo_wait_limit_s(const SpmvAmdCgSlab* s) { return halo_wait_limit_s(s->wait_limit_s, watchdog_limit_seconds()); }

// The slab's first and last grid row (the rows that read the halos) on `stream`; partial slots follow the
// interior launch's. Returns the number of partials written (0 without partials).
static int slab_boundary_spmv(SpmvAmdCgSlab* s, const double* in, double* part, const int* skip, hipStream_t stream, const ResidualOut* init) {
    const SlabCsr& A = s->A.view;
    const auto [lo, hi] = s->halo_free();
    double* at = part ? part + (hi > lo ? s->plan_interior.partials : 0) : nullptr;
    int used = 0;
    if (lo > 0 && hi < s->n_local && lo == A.grid_size && s->n_local - hi == A.grid_size) {
        // a rank with two neighbours: its first and last grid row in one launch
        used += launch_stencil5_spmv_first_and_last_gridrow(A, s->plan_head, s->plan_tail, in, s->Ap, 1.0, at, skip, stream, init, s->sym());
    } else {
        if (lo > 0) used += launch_stencil5_spmv(A, s->plan_head, in, s->Ap, 1.0, at, skip, false, stream, init, s->sym());
        if (hi < s->n_local)
            used += launch_stencil5_spmv(A, s->plan_tail, in, s->Ap, 1.0, at ? at + used : nullptr, skip, false, stream, init, s->sym());
    }
    return part ? used : 0;
}

// Sum of the partials the last slab_spmv wrote (`used` of them): a split SpMV's boundary-row partials as extra values.
// partials (null: partials_spmv): the array the launches wrote, where it is another one (slab_first_spmv's b.b partials).
void reduce_spmv_partials(SpmvAmdCgSlab* s, int used, double* d_out, const int* skip, int* progress, int progress_value, const PeerMailbox* mailbox,
                          const double* partials) {
    if (partials == nullptr) partials = s->partials_spmv;
    const int first = s->spmv_split_at >= 0 && s->spmv_split_at < used ? s->spmv_split_at : used;
    launch_reduce_partials(partials, first, d_out, skip, s->compute, s->scratch(), progress, progress_value, mailbox, partials + first, used - first);
}

// SpMV of the slab on p (halos must be current or in flight on the side stream).
// overlap = the halo exchange was started on the side stream and ev_halo_done marks its end.
// spmv_done (optional): recorded behind the last SpMV launch, before the reduction of its partials.
// init (may be null): the launches write r = b - A x, p = r and r.r partials instead of A x (fused initial residual);
// the caller reduces the partials. x_zero (with init, on a slab without neighbours that owns its matrix): `input` holds zeros the
// library wrote, see launch_stencil5_spmv. ap_not_stored (LoopShape::first_recomputed, iteration 0 on a caller's x0): the whole-slab
// block launch leaves A p unstored on its fast blocks; only a slab whose SpMV is that one launch may ask.
// Returns the number of partial slots the launches wrote.
int slab_spmv(SpmvAmdCgSlab* s, bool with_dot, bool overlap, const int* skip, const double* input, hipEvent_t spmv_done,
              const ResidualOut* init, bool x_zero, bool ap_not_stored) {
    const SlabCsr& A = s->A.view;
    const double* in = input ? input : s->p;
    double* part = ((with_dot && s->fused_dot) || init) ? s->partials_spmv : nullptr;
    const auto [lo, hi] = s->halo_free();
    int used = 0;
    s->spmv_split_at = -1;
    if (ap_not_stored && (s->op != nullptr || lo != 0 || hi != s->n_local)) {
        fprintf(stderr, "[cg-slab] only the whole-slab block launch can leave A p unstored\n");
        exit(EXIT_FAILURE);
    }
    if (s->op != nullptr) {
        // the caller's operator: its fused launch when it has one (this library's stencil5-csr), else the vtable
        if (part != nullptr) {
            used = s->fused.launch(in, s->Ap, part, skip, s->shape.reverse, init, s->compute);
        } else if (s->op->run_device(in, s->Ap) != 0) {
            // The reference ignores this return value (cg_solver.cu:498,541); a library must not end its caller's process
            // over it either: remember it, let the solve wind down and hand the failure back as a status.
            fprintf(stderr, "[cg] operator '%s': run_device failed\n", s->op->name);
            s->op_failed = true;
        }
        if (s->tl_after_interior) HIP_CHECK(hipEventRecord(s->tl_after_interior, s->compute));
    } else if (hi <= lo || (lo == 0 && hi == s->n_local) || (part == nullptr && !overlap)) {
        // one launch: a slab without halo rows, or of one or two grid rows, or a plain y = A x with the halos already in place
        if (overlap) HIP_CHECK(hipStreamWaitEvent(s->compute, s->ev_halo_done, 0));
        used = launch_stencil5_spmv(A, s->plan_whole, in, s->Ap, 1.0, part, skip, s->shape.reverse, s->compute, init, s->sym(), x_zero, ap_not_stored);
        if (s->tl_after_interior) HIP_CHECK(hipEventRecord(s->tl_after_interior, s->compute));
    } else {
        // rows whose north and south neighbours are local run under the halo exchange; the first / last grid row of the slab once
        // the halo rows have landed. A launch that writes dot partials is split in this way even when the exchange is NOT
        // overlapped (detailed timers, SPMV_AMD_NO_OVERLAP): the sum's shape -- slices of the interior partials, then [slice sums |
        // boundary rows' partials] -- must not depend on how the halos travelled. (The boundary rows on the side stream, or the
        // halo wait in front of the interior launch, measured slower: DESIGN §8.)
        used = launch_stencil5_spmv(A, s->plan_interior, in, s->Ap, 1.0, part, skip, s->shape.reverse, s->compute, init, s->sym());
        s->spmv_split_at = used;  // the boundary rows' partials follow: they enter the sum as extra values (reduce_device.hpp)
        if (s->tl_after_interior) HIP_CHECK(hipEventRecord(s->tl_after_interior, s->compute));
        // in-loop SpMV: the boundary rows ride in the launch that reduces the partials (one launch instead of three); the
        // launch timer and the timeline's boundary-row mark then stop behind the interior rows (all but one or two grid rows
        // of the slab), and the stage "reduce_pAp" holds the halo wait, the boundary rows and the sum
        const bool fused_tail = slab::fused_tail(with_dot, part != nullptr, init != nullptr, lo, s->n_local - hi, A.grid_size);
        if (fused_tail && spmv_done) HIP_CHECK(hipEventRecord(spmv_done, s->compute));
        HaloArrival arrival;
        if (fused_tail && overlap) {
            // the boundary waves wait for the exchange's arrival flag themselves; bounded well inside the host's watchdog
            arrival = HaloArrival{s->d_halo_flag, s->halo_sequence, (long long)(halo_wait_limit_s(s) * 1e8), &s->h_poll->halo_late};
        } else if (overlap) {
            HIP_CHECK(hipStreamWaitEvent(s->compute, s->ev_halo_done, 0));
        }
        if (fused_tail && launch_stencil5_edges_and_reduce(A, s->plan_interior, lo > 0, hi < s->n_local, in, s->Ap, 1.0, part, &s->d_s->pAp, skip,
                                                           s->scratch(), s->spmv_progress, s->spmv_progress_value, s->reduce_mailbox, s->compute,
                                                           arrival, s->sym())) {
            return used;
        }
        if (arrival.flag != nullptr) HIP_CHECK(hipStreamWaitEvent(s->compute, s->ev_halo_done, 0));  // the fused launch did not apply
        if (fused_tail) spmv_done = nullptr;  // already recorded
        used += slab_boundary_spmv(s, in, part, skip, s->compute, init);
    }
    if (spmv_done) HIP_CHECK(hipEventRecord(spmv_done, s->compute));
    if (with_dot) {
        if (part)
            reduce_spmv_partials(s, used, &s->d_s->pAp, skip, s->spmv_progress, s->spmv_progress_value, s->reduce_mailbox);
        else
            launch_dot((size_t)s->n_local, s->p, s->Ap, s->partials_blas, &s->d_s->pAp, s->compute);
    }
    return used;
}

// p_out = r + beta p_in, Ap = A p_out, the partials of p_out . Ap and their sum: the direction update of iteration `iteration`
// (1-based, as the kernels count) and the SpMV of the next one in one launch (+ one over the slow blocks), on a slab without
// neighbours. spmv_done as in slab_spmv.
int slab_direction_spmv(SpmvAmdCgSlab* s, const double* p_in, double* p_out, int iteration, hipEvent_t spmv_done, bool ap_not_stored) {
    s->spmv_split_at = -1;
    const DirectionSpmv d{s->d_s, iteration, s->device_form, s->r, p_in, p_out, s->slow_list_whole, s->slow_count_whole, ap_not_stored};
    const int used = launch_stencil5_direction_spmv(s->A.view, s->plan_whole, d, s->Ap, 1.0, s->partials_spmv, s->shape.reverse, s->compute, *s->sym());
    if (s->tl_after_interior) HIP_CHECK(hipEventRecord(s->tl_after_interior, s->compute));
    if (spmv_done) HIP_CHECK(hipEventRecord(spmv_done, s->compute));
    reduce_spmv_partials(s, used, &s->d_s->pAp, &s->d_s->converged, s->spmv_progress, s->spmv_progress_value, s->reduce_mailbox);
    return used;
}

// The r update behind a slab_direction_spmv that did not store A p' on its fast blocks (LoopShape::ap_recomputed): r -= alpha A p_new
// with the r.r partials into partials_blas, cg_update_r_kernel's slots. Returns the partial count. r_is_p (iteration 0 under
// LoopShape::first_recomputed, p_new = b or ring slot 0): r = p_new - alpha A p_new, out of place.
int slab_update_r_recompute(SpmvAmdCgSlab* s, const double* p_new, bool reverse, bool r_is_p) {
    return launch_cg_update_r_recompute(s->A.view, s->plan_whole, s->d_s, p_new, s->Ap, s->r, s->partials_blas, s->row_block_fast, reverse, s->compute,
                                        *s->sym(), r_is_p);
}

static const char* query_name(hipError_t e) {
    return e == hipSuccess ? "idle (all work done)" : e == hipErrorNotReady ? "busy (work pending)" : hipGetErrorString(e);
}

// What the watchdog prints about a slab whose rank stopped making progress. Runs on the watchdog's thread;
// queries only.
void report_slab_state(void* user, FILE* out) {
    const SpmvAmdCgSlab* s = static_cast<const SpmvAmdCgSlab*>(user);
    const int seq = __atomic_load_n(&s->h_poll->sequence, __ATOMIC_ACQUIRE);
    const int prog = __atomic_load_n(&s->h_poll->progress, __ATOMIC_ACQUIRE);
    fprintf(out, "[cg-slab] rank %d (slab %d of %d, rows [%d, %d)): last work enqueued by the host: %s of iteration %d\n",
            s->comm->rank, s->part_rank, s->part_world, s->row_offset, s->row_offset + s->n_local, s->enqueued_stage,
            s->enqueued_iteration);
    fprintf(out, "[cg-slab] status records: waiting for #%d, GPU has published #%d (iterations counted %d, converged %d)\n",
            s->poll_sequence, seq, s->h_poll->iterations, s->h_poll->converged);
    const char* where = "before the local p.Ap sum: in the SpMV, or waiting for the halo rows (see the events below)";
    if (prog == 4 * s->poll_sequence + 1)
        where = "local p.Ap summed: in the all-reduce of p.Ap, the r update or the local r.r sum";
    else if (prog == 4 * s->poll_sequence + 2)
        where = "local r.r summed: in the all-reduce of r.r or the scalar step";
    if (seq != s->poll_sequence) fprintf(out, "[cg-slab] GPU progress inside that iteration: %s\n", where);
    fprintf(out, "[cg-slab] compute stream: %s; side (halo) stream: %s\n", query_name(hipStreamQuery(s->compute)),
            query_name(hipStreamQuery(s->side)));
    fprintf(out, "[cg-slab] event 'direction vector ready for the halo exchange': %s; event 'halo rows received': %s\n",
            query_name(hipEventQuery(s->ev_p_ready)), query_name(hipEventQuery(s->ev_halo_done)));
    s->comm->describe(out);
}

// Has the scalar step that publishes record `sequence` run? (Records carry increasing sequence numbers, one per iteration, over
// the life of the slab; a later record implies the earlier ones.)
static bool record_arrived(const SpmvAmdCgSlab* s, int sequence) {
    return (int)(__atomic_load_n(&s->h_poll->sequence, __ATOMIC_ACQUIRE) - sequence) >= 0;
}

// Blocks the host until record `sequence` has been published. Bounded by the watchdog (SPMV_AMD_WATCHDOG_S): a rank whose
// peers never answer ends with a report, not a hang.
static void wait_for_record(SpmvAmdCgSlab* s, int sequence) {
    if (record_arrived(s, sequence)) return;
    WatchdogScope guard("waiting for the iteration's status record", s->comm->rank, s->enqueued_iteration,
                        report_slab_state, s);
    long spins = 0;
    while (!record_arrived(s, sequence)) {
        __builtin_ia32_pause();  // the record arrives within one iteration; the spinning core at least yields its pipeline
        if (++spins % (1L << 20) == 0) {
            // surface a faulted stream at once instead of waiting for the watchdog
            const hipError_t e = hipStreamQuery(s->compute);
            if (e != hipSuccess && e != hipErrorNotReady) HIP_CHECK(e);
            if (e == hipSuccess && !record_arrived(s, sequence)) {
                fprintf(stderr, "[cg-slab] status record missing after the stream drained\n");
                exit(EXIT_FAILURE);
            }
        }
    }
}

// Halo rows of a halo-carrying vector v (local part at v): first / last grid row to the neighbours, theirs
// into [v - halo, v) and [v + n_local, v + n_local + halo).
static void exchange_halo(SpmvAmdCgSlab* s, double* v, hipStream_t stream) {
    if (!s->comm->exchanges_halos()) return;
    // a staged transport blocks in here on its host exchange, RCCL may block while it connects peers
    WatchdogScope guard("halo exchange (send/recv of the first and last grid row)", s->comm->rank, s->enqueued_iteration, report_slab_state, s);
    // LAB build, SPMV_AMD_TEST_WEDGE_OVERLAPPED_EXCHANGE=1 (test hook): an exchange issued on the SIDE stream never returns, as behind
    // an RCCL call that blocks -- the watchdog ends the process and a supervisor can be shown to restart the ranks without the overlap
    // (tests/test_distributed.py); nothing is wedged on the GPU. = 2: the exchange returns, but a pipeline that overlaps delivers
    // WRONG NUMBERS (the right-hand side is nudged once): what a hand-over that loses rows would look like to the supervisor.
#ifdef SPMV_AMD_LAB
    while (s->test_wedge_overlapped_exchange == 1 && stream == s->side && s->side != nullptr) std::this_thread::sleep_for(std::chrono::milliseconds(200));
    if (s->test_wedge_overlapped_exchange == 2 && stream == s->side && s->side != nullptr) {
        static const double nudged = 1.001;
        HIP_CHECK(hipMemcpyAsync(s->b, &nudged, sizeof nudged, hipMemcpyHostToDevice, stream));
        s->test_wedge_overlapped_exchange = 0;
    }
    // = 3: the rows of a side-stream exchange never travel (the halos keep what they held) -- what the creation check
    // (verify_pipeline) must notice; = 4: the exchange runs but its arrival flag is never raised (SolveRun::start_halo)
    if (s->test_wedge_overlapped_exchange == 3 && stream == s->side && s->side != nullptr) return;
#endif
    s->comm->halo_exchange(s->has_prev ? v : nullptr, s->has_next ? v + (s->n_local - s->halo) : nullptr,
                           s->has_prev ? v - s->halo : nullptr, s->has_next ? v + s->n_local : nullptr, s->halo, stream);
}
static void allreduce_scalar(SpmvAmdCgSlab* s, double* d_value, const char* stage) {
    if (s->comm->mailbox_ready()) {  // stores between the GPUs, one small launch, nothing for the host to wait on
        launch_mailbox_allreduce(s->comm, d_value, s->compute);
        return;
    }
    WatchdogScope guard(stage, s->comm->rank, s->enqueued_iteration, report_slab_state, s);
    s->comm->allreduce_sum(d_value, 1, s->compute);
}

// What the loop's shape is decided from (slab_decisions.hpp, loop_shape): the slab and its communicator as plain values.
ShapeInputs shape_inputs(const SpmvAmdCgSlab* s, bool detailed_timers) {
    const SpmvAmdComm* comm = s->comm;
    const Stencil5Plan& p = s->plan_whole;
    const SymPlanes* sp = s->sym();
    ShapeInputs in{};
    in.exchanges_halos = comm->exchanges_halos(), in.collective = comm->collective(), in.mailbox_ready = comm->mailbox_ready();
    in.detailed_timers = detailed_timers;
    in.ring_slots = s->ring_slots, in.n_local = (size_t)s->n_local, in.halo = s->halo, in.has_prev = s->has_prev, in.has_next = s->has_next;
    in.owns_matrix = s->op == nullptr, in.no_overlap = s->no_overlap, in.reduce_scratch = s->reduce_stage != nullptr;
    in.fused_direction = s->fused_direction;
    // the direction update inside the block SpMV (kernels.hpp, DirectionSpmv): the plan runs the block kernel on the class map
    in.fused_dot = s->fused_dot, in.planes_and_classes = sp != nullptr && sp->ce != nullptr && sp->cls != nullptr;
    in.block_plan = p.variant == Stencil5Variant::RowLds && p.block_rows > 0 && p.block_map != nullptr;
    in.slow_blocks = s->slow_count_whole, in.block_tiles = in.block_plan ? rowlds_block_tiles(p) : 0;
    in.late_bulk = s->late_bulk, in.fuse_init_residual = s->fuse_init_residual, in.x0_known_zero = s->x0_known_zero;
    in.zero_start_parts = s->zero_start_mask();
    in.zero_rows_plus_zero = s->zero_rows_plus_zero;
    in.ap_recompute = s->ap_recompute, in.skew_eligible = s->skew_eligible && s->row_block_fast != nullptr;
    in.first_recompute = s->first_recompute;
    return in;
}

// The first SpMV of a solve on a slab that takes the initial residual from it (fuse_init_residual): r0 = b - A x0 into ring slot 0
// (p0) and, unless the shape keeps it there alone, into r; the r0.r0 partials into partials_spmv. Returns the partial slots written.
int slab_initial_residual(SpmvAmdCgSlab* s, const LoopShape& L, bool halo_in_flight) {
    const ResidualOut init{s->b, L.r0_in_ring ? nullptr : s->r, s->ring[0]};
    return slab_spmv(s, /*with_dot=*/false, halo_in_flight, nullptr, s->x0, nullptr, &init, L.zero_start);
}

// LoopShape::b_is_p0: iteration 0's SpMV on b -- Ap = A b, the b.Ab partials into partials_spmv and the b.b partials into
// partials_first, one launch -- with the marks slab_spmv leaves behind a one-launch SpMV. The caller reduces both arrays.
int slab_first_spmv(SpmvAmdCgSlab* s, bool reverse, hipEvent_t spmv_done, bool ap_not_stored) {
    s->spmv_split_at = -1;
    const int used = launch_stencil5_first_spmv(s->A.view, s->plan_whole, s->b, s->Ap, 1.0, s->partials_spmv, s->partials_first, reverse, s->compute, *s->sym(),
                                                ap_not_stored);
    if (s->tl_after_interior) HIP_CHECK(hipEventRecord(s->tl_after_interior, s->compute));
    if (spmv_done) HIP_CHECK(hipEventRecord(spmv_done, s->compute));
    return used;
}

// One solve. The loop has TWO shapes, fixed per solve (LoopShape): the pipeline and the plain order; an iteration is the
// same five stages in both -- SpMV (+ p.Ap sum) | all-reduce | r update | r.r sum (+ all-reduce) + scalar step | direction
// update + halo exchange -- and each stage is one function below. What a stage enqueues depends on the shape only.
namespace {

// State of one solve in flight: what the stages share.
struct SolveRun {
    SpmvAmdCgSlab* s;
    const CGConfigMultiGPU* config;
    CGStatsMultiGPU* stats;
    const LoopShape L;
    // L.b_is_p0 in a solve that runs iteration 0: b stands for ring slot 0 until the ring wraps, and iteration 0's SpMV is enqueued
    // by initial_residual (a solve of no iterations keeps the launch that only sums r0.r0)
    const bool b_is_p0;
    const FirstForm first;  // iteration 0's A p0: stored and read back, or left unstored and recomputed by its r update (first_form)
    const PeerMailbox* const mailbox;  // non-null: the communicator's peer mailbox completes the sums (L.use_mailbox)
    const EdgeRows edges;              // pipeline: the rows the neighbours wait for, [0, count_a) and [second, second + count_b)
    const TraceRanges trace;
    EventTimer total, part;
    const size_t nl;
    const int* skip;
    const bool timeline;
    RingSlots ring_view;
    int window_start = 0;       // first iteration whose alpha_k p_k is not in x yet (ring mode)
    int tl_exchanges = 0;       // halo exchanges marked on the side stream (exchange j precedes the SpMV of iteration j)
    bool halo_in_flight = false;
    bool step_in_direction = false;  // this iteration's scalar step rides in the direction update's launch
    const double* direction_from = nullptr;  // fused_direction: p of the iteration just stepped, which the next SpMV launch reads r + beta p from
    // Status records: the record of iteration j (1-based) of this solve carries sequence0 + j. records_read = the latest
    // iteration whose record the host has seen; the host runs at most ONE iteration ahead of it (read_status).
    int sequence0 = 0, records_read = 0;
    bool backward = false;      // sweep direction of this iteration's SpMV and direction update (the r update walks the other way)
    int enqueued = 0, sampled = 0;
    std::vector<int> sampled_iteration;  // 0-based loop index of each timed SpMV

    SolveRun(SpmvAmdCgSlab* slab, const CGConfigMultiGPU* cfg, CGStatsMultiGPU* st)
        : s(slab), config(cfg), stats(st), L(loop_shape(slab, cfg->enable_detailed_timers != 0)), b_is_p0(L.b_is_p0 && cfg->max_iters > 0), first(first_form(L, cfg->max_iters)),
          mailbox(L.use_mailbox ? slab->comm->d_mailbox : nullptr),
          edges{L.head_rows, L.tail_start, L.pipeline ? (size_t)slab->n_local - L.tail_start : 0}, trace(L.detail || slab->roctx_always), nl((size_t)slab->n_local),
          skip(&slab->d_s->converged), timeline(slab->timeline_on && !L.detail) {
        for (int k = 0; k < kMaxRingSlots; ++k) ring_view.p[k] = s->ring[(size_t)k % s->ring.size()];
    }

    // detailed timers (the reference's, :770-800): a stage between two events and a host sync; otherwise just the stage
    template <class Work>
    void timed(double* bucket, double* bucket2, Work&& work) {
        if (!L.detail) {
            work();
            return;
        }
        part.begin(s->compute);
        work();
        part.end(s->compute);
        WatchdogScope guard("detailed timers: waiting for the stage just enqueued", s->comm->rank, s->enqueued_iteration, report_slab_state, s);
        const double ms = part.elapsed_ms();
        if (bucket) *bucket += ms;
        if (bucket2) *bucket2 += ms;
    }
    static hipEvent_t tl_event(std::vector<hipEvent_t>& pool, size_t index) {
        while (pool.size() <= index) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            pool.push_back(e);
        }
        return pool[index];
    }
    // compute-stream marks: [0] solve start, [1] initial residual done, then kTimelineMarks per iteration, then the flush
    size_t mark_index(int iteration, int k) const { return 2 + (size_t)iteration * kTimelineMarks + k; }
    void mark(int iteration, int k) {
        if (timeline) HIP_CHECK(hipEventRecord(tl_event(s->tl_compute, mark_index(iteration, k)), s->compute));
    }

    // the ring as a flush reads it: in the solve's first window b is slot 0 where it serves as p0 (the real slot 0 is written when
    // the ring wraps, behind the flush of that window)
    RingSlots flush_ring() const {
        RingSlots v = ring_view;
        if (b_is_p0 && window_start == 0) v.p[0] = s->b;
        return v;
    }
    // the event pair around every spmv_event_stride-th in-loop SpMV: is iteration `index` (0-based) one of them, and its pair
    bool samples(int index) const { return !timeline && !L.detail && s->spmv_event_stride > 0 && (index + s->spmv_event_phase) % s->spmv_event_stride == 0; }
    hipEvent_t* sample_pair() {
        while (s->spmv_ev.size() < 2 * (size_t)(sampled + 1)) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            s->spmv_ev.push_back(e);
        }
        return &s->spmv_ev[2 * (size_t)sampled];
    }
    // what a flush of x starts from: x itself, the stored x0 for the solve's first window -- or nothing (null: the chain starts from
    // 0.0 in registers) where x0 holds the library's own zeros
    const double* flush_from() const { return window_start > 0 ? s->x : (flush_skips_x0(s->x0_known_zero, s->zero_start_mask()) ? nullptr : s->x0); }
    // what the host knows of this solve, for the run-ahead rules; the LAB build's hooks are constants in the product
    StatusView status() const {
#ifdef SPMV_AMD_LAB
        return StatusView{s->d_hist, s->hist_cap, config->tolerance, LabHooks{s->stop_at, s->guess_far_always}};
#else
        return StatusView{s->d_hist, s->hist_cap, config->tolerance, LabHooks{}};
#endif
    }

    void begin();
    void initial_residual();
    void start_halo(double* v, bool released_by_flag);
    void stage_spmv();
    void stage_allreduce_pAp();
    void stage_update_r();
    void stage_sum_rr_and_step();
    void stage_direction_and_halo();
    void await_record(int iteration);
    bool read_status();
    void finish();
    void resolve_timeline(const CgScalars& fin, float total_ms);
};

void SolveRun::begin() {
    s->reduce_mailbox = nullptr;  // the initial SpMV has no dot product
    s->op_failed = false;
    s->last_ap_recomputed = L.ap_recomputed, s->last_recompute_launches = 0, s->last_first_form = (int)first;
    memset(stats, 0, sizeof(*stats));
    // residual history: one slot per iteration, capped at 2^20 entries (later iterations go unrecorded)
    const int want_hist = slab::want_hist(config->max_iters);
    if (s->hist_cap < want_hist) {
        // host-coherent pinned memory, written by the scalar kernels one 8-byte store per iteration: the host reads the history
        // (and with it the final residual) where it lies, no copy command at the end of a solve
        if (s->d_hist) HIP_CHECK(hipHostFree(s->d_hist));
        s->hist_cap = want_hist;
        HIP_CHECK(hipHostMalloc((void**)&s->d_hist, (size_t)s->hist_cap * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
    }
    CgScalars init;
    memset(&init, 0, sizeof init);
    init.max_history = s->hist_cap;
#ifdef SPMV_AMD_LAB
    init.stop_at = s->stop_at;
#endif
    HIP_CHECK(hipMemcpyAsync(s->d_s, &init, sizeof init, hipMemcpyHostToDevice, s->compute));
#ifdef SPMV_AMD_LAB
    poison_halos(s);  // the lab's tests solve one system again and again: a row that did not travel must not find last solve's copy
#endif
    // Every solve starts from the stored x0 (the reference benchmark wrapper restores x on the host before each run). x is not
    // overwritten with x0 first: the initial SpMV reads x0 and the first x update computes x = x0 + alpha p.
    HIP_CHECK(hipStreamSynchronize(s->compute));
    s->timeline_us.clear();
    s->p = b_is_p0 ? s->b : s->ring[0];  // b as p0: what the direction update of iteration 1 reads (never written: p_next is a ring slot)
    sequence0 = s->poll_sequence;
    records_read = 0;
    s->h_poll->converged = 0, s->h_poll->iterations = 0;  // (the stream is idle: nothing of the previous solve can still write here)
    s->enqueued_stage = "barrier before the timed region";
    s->enqueued_iteration = -1;
    {
        WatchdogScope guard("barrier before the timed region", s->comm->rank, -1, report_slab_state, s);
        s->comm->barrier(s->compute);
    }
    total.begin(s->compute);
    if (timeline) HIP_CHECK(hipEventRecord(tl_event(s->tl_compute, 0), s->compute));
}

// Halo rows of the halo-carrying vector v to / from the neighbours. PIPELINE: on the side stream, behind the rows to send --
// released by the direction launch's device flag (released_by_flag: the edge rows were written through by that launch's first
// workgroups; no event on the compute stream, and not as late as the launch's end) or by an event (x0's rows at the start of
// a solve) -- and followed by the arrival flag the boundary waves wait for and the event everything else waits for.
// PLAIN: on the compute stream, in order.
void SolveRun::start_halo(double* v, bool released_by_flag) {
    if (!L.multi) return;
    if (!L.pipeline) {
        timed(&stats->time_allgather_ms, nullptr, [&] { exchange_halo(s, v, s->compute); });
        halo_in_flight = false;
        return;
    }
    if (released_by_flag) {
        launch_edges_wait(s->scratch(), s->poll_sequence, (long long)(halo_wait_limit_s(s) * 1e8), &s->h_poll->halo_late, s->side);
    } else {
        HIP_CHECK(hipEventRecord(s->ev_p_ready, s->compute));
        HIP_CHECK(hipStreamWaitEvent(s->side, s->ev_p_ready, 0));
    }
    const bool in_loop = v != s->x0;
    if (timeline && in_loop) HIP_CHECK(hipEventRecord(tl_event(s->tl_side, 2 * (size_t)tl_exchanges), s->side));
    exchange_halo(s, v, s->side);
    ++s->halo_sequence;
#ifdef SPMV_AMD_LAB
    if (s->test_wedge_overlapped_exchange != 4)  // fault injection: an arrival flag that never comes
#endif
        launch_halo_arrived(s->d_halo_flag, s->halo_sequence, s->side);
    if (timeline && in_loop) HIP_CHECK(hipEventRecord(tl_event(s->tl_side, 2 * (size_t)tl_exchanges++ + 1), s->side));
    HIP_CHECK(hipEventRecord(s->ev_halo_done, s->side));
    halo_in_flight = true;
}

// ---- r0 = b - A x0 ; p0 = r0 ; rr0 ----
// x0 is read where it lies: its allocation carries the halo rows the first / last grid row need (its halo rows travel like
// p's, so that the point-to-point communicator is driven from one stream only).
void SolveRun::initial_residual() {
    start_halo(s->x0, /*released_by_flag=*/false);
    int first_used = 0;
    if (b_is_p0) {
        // r0 is b and p0 is b: nothing to compute or store. Iteration 0's SpMV goes first, on b, in that iteration's sweep direction
        // (the r update behind it starts where it ends), and sums b.b on its way; it is that iteration's SpMV for the launch timers.
        hipEvent_t spmv_done = nullptr;
        if (samples(0)) {
            hipEvent_t* pair = sample_pair();
            HIP_CHECK(hipEventRecord(pair[0], s->compute));
            spmv_done = pair[1];
        }
        first_used = slab_first_spmv(s, sweeps_backward(0), spmv_done, first != FirstForm::Stored);
        reduce_spmv_partials(s, first_used, &s->d_s->rr_new, nullptr, nullptr, 0, mailbox, s->partials_first);
    } else if (s->fuse_init_residual) {
        // row-lds slabs: r0 = b - A x0, p0 = r0 and the r0.r0 partials come out of the SpMV launch itself (A x0 is
        // never written out and read back: 16 B/row less, once per solve)
        int used = 0;
        timed(&stats->time_initial_r_ms, nullptr, [&] { used = slab_initial_residual(s, L, halo_in_flight); });
        timed(&stats->time_dot_rs_initial_ms, nullptr, [&] { reduce_spmv_partials(s, used, &s->d_s->rr_new, nullptr, nullptr, 0, mailbox); });
    } else {
        slab_spmv(s, /*with_dot=*/false, halo_in_flight, nullptr, s->x0);
        timed(&stats->time_initial_r_ms, nullptr, [&] { launch_cg_init_residual(nl, s->b, s->Ap, s->r, s->p, s->partials_blas, s->compute); });
        timed(&stats->time_dot_rs_initial_ms, nullptr, [&] {
            launch_reduce_partials(s->partials_blas, cg_partial_count(nl), &s->d_s->rr_new, nullptr, s->compute, s->scratch(), nullptr, 0, mailbox);
        });
    }
    s->enqueued_stage = "initial residual";
    if (L.separate) allreduce_scalar(s, &s->d_s->rr_new, "all-reduce of the initial r.r");
    s->reduce_mailbox = s->fused_dot ? mailbox : nullptr;  // the in-loop SpMVs' p.Ap reduction
    launch_cg_scalars_init(s->d_s, s->d_hist, s->compute);
    // b as p0: the b.Ab sum of iteration 0, behind the scalars' initialisation as the in-loop reduction is (it tests the flag that sets)
    if (b_is_p0) reduce_spmv_partials(s, first_used, &s->d_s->pAp, skip, &s->h_poll->progress, 4 * (s->poll_sequence + 1) + 1, s->reduce_mailbox);
    if (timeline) HIP_CHECK(hipEventRecord(tl_event(s->tl_compute, 1), s->compute));
    if (s->label && config->verbose >= 1) {  // the reference prints ||r0|| before its loop (cg_solver.cu:529-531); verbose runs only
        CgScalars now;
        HIP_CHECK(hipStreamSynchronize(s->compute));
        HIP_CHECK(hipMemcpy(&now, s->d_s, sizeof now, hipMemcpyDeviceToHost));
        printf("[%s] Initial residual: %e\n", s->label, now.b_norm);
    }
    start_halo(s->p, /*released_by_flag=*/false);  // halo rows of p0: under the first interior SpMV
}

// Stage 1: Ap = A p with the p.Ap partials and their sum (slab_spmv: interior rows | boundary rows + sum on a split slab).
void SolveRun::stage_spmv() {
    // SpMV and direction update of iteration k walk one way, the r update between them the other way; the direction flips
    // every iteration, so every kernel starts where the previous one ended (iteration 0 follows the forward initial pass)
    backward = sweeps_backward(enqueued);
    s->shape.reverse = backward;
    s->enqueued_iteration = enqueued;
    s->enqueued_stage = "SpMV";
    TraceScope range(trace, "SpMV");
    s->spmv_progress = &s->h_poll->progress;
    s->spmv_progress_value = 4 * (s->poll_sequence + 1) + 1;
    mark(enqueued, 0);
    // fused_direction: the launch of iterations >= 1 writes this iteration's direction (s->p, the slot the direction stage chose)
    // from the previous one on its way; `enqueued` is the number of the iteration that direction belongs to, as the kernels count
    const auto spmv = [&](hipEvent_t spmv_done) {
        if (L.fused_direction && enqueued > 0) return slab_direction_spmv(s, direction_from, s->p, enqueued, spmv_done, L.ap_recomputed);
        // (iteration 0 under first_recomputed: the block kernel leaves A p0 to the r update too)
        return slab_spmv(s, true, halo_in_flight, skip, nullptr, spmv_done, nullptr, false, enqueued == 0 && first != FirstForm::Stored);
    };
    if (b_is_p0 && enqueued == 0) {
        // initial_residual enqueued this iteration's launch and the reduction of its partials (with the event pair where this is a
        // timed iteration): the timeline's SpMV marks of iteration 0 enclose nothing, its launch lies in initial_residual_us
        if (timeline) mark(0, 1), mark(0, 2);
        else if (samples(0)) sampled_iteration.push_back(0), ++sampled;
    } else if (timeline) {
        // [1] is recorded inside slab_spmv behind the interior launch, [2] behind the boundary rows; the reduction of the
        // partials is issued by slab_spmv too, so [3] follows directly
        s->tl_after_interior = tl_event(s->tl_compute, mark_index(enqueued, 1));
        spmv(tl_event(s->tl_compute, mark_index(enqueued, 2)));
        s->tl_after_interior = nullptr;
    } else if (L.detail) {
        timed(&stats->time_spmv_ms, nullptr, [&] { spmv(nullptr); });
    } else if (samples(enqueued)) {
        hipEvent_t* pair = sample_pair();
        HIP_CHECK(hipEventRecord(pair[0], s->compute));
        spmv(pair[1]);
        sampled_iteration.push_back(enqueued);
        ++sampled;
    } else {
        spmv(nullptr);
    }
    s->spmv_progress = nullptr;
}

// Stage 2 (only where the sum is not completed across the ranks inside the reduction's launch).
void SolveRun::stage_allreduce_pAp() {
    s->enqueued_stage = "all-reduce of p.Ap";
    if (L.separate || (L.reduce && !s->fused_dot)) {
        TraceScope r(trace, "AllReduce");
        timed(&stats->time_allreduce_ms, nullptr, [&] { allreduce_scalar(s, &s->d_s->pAp, "all-reduce of p.Ap"); });
    }
    mark(enqueued, 3);
}

// Stage 3: r -= alpha Ap with the r.r partials (alpha = rr_old / pAp in every thread).
void SolveRun::stage_update_r() {
    s->enqueued_stage = "r update";
    TraceScope range(trace, "BLAS_AXPY");
    timed(&stats->time_blas1_ms, &stats->time_axpy_update_r_ms,
          [&] {
              // r0_in_ring: r0 lies in ring slot 0 alone (p0 = r0, stored once): the update of iteration 0 reads it there
              // (b_is_p0: r0 is b itself)
              // ap_recomputed: the fused launch of iterations >= 1 left A p' unstored on its fast blocks; s->p is the p' it wrote
              // first_recomputed: iteration 0's launch left A p0 unstored as well; r0 is b, or slot 0, or -- stored twice -- already in r
              if (L.ap_recomputed && enqueued > 0) slab_update_r_recompute(s, s->p, !backward), ++s->last_recompute_launches;
              else if (enqueued == 0 && first == FirstForm::FromB) slab_update_r_recompute(s, s->b, !backward, /*r_is_p=*/true);
              else if (enqueued == 0 && first == FirstForm::FromSlot0) slab_update_r_recompute(s, s->ring[0], !backward, /*r_is_p=*/true);
              else if (enqueued == 0 && first == FirstForm::InPlace) slab_update_r_recompute(s, s->p, !backward);
              else if (L.r0_in_ring && enqueued == 0) launch_cg_update_r_from(nl, s->d_s, s->Ap, b_is_p0 ? s->b : s->ring[0], s->r, s->partials_blas, s->compute, !backward);
              else launch_cg_update_r(nl, s->d_s, s->Ap, s->r, s->partials_blas, s->compute, !backward);
          });
    mark(enqueued, 4);
}

// Stage 4: sum of the r.r partials, across the ranks, and the scalar step (residual, history, verdict, beta, alpha into the
// ring's slot, status record into host-coherent memory). One launch without a separate all-reduce; with one (RCCL) the
// step follows the all-reduce -- as a launch of its own, or inside the direction update's launch (step_in_direction).
void SolveRun::stage_sum_rr_and_step() {
    step_in_direction = slab::step_in_direction(L.pipeline, L.separate, enqueued, window_start, L.slots);
    ++s->poll_sequence;
    TraceScope range(trace, "Dot_Product");
    if (L.separate) {
        timed(&stats->time_reductions_ms, &stats->time_dot_rs_new_ms, [&] {
            launch_reduce_partials(s->partials_blas, cg_partial_count(nl), &s->d_s->rr_new, skip, s->compute, s->scratch(), &s->h_poll->progress,
                                   4 * s->poll_sequence + 2);
        });
        s->enqueued_stage = "all-reduce of r.r";
        {
            TraceScope r(trace, "AllReduce");
            timed(&stats->time_allreduce_ms, nullptr, [&] { allreduce_scalar(s, &s->d_s->rr_new, "all-reduce of r.r"); });
        }
        if (!step_in_direction)
            launch_cg_scalars_step(s->d_s, config->tolerance, s->d_hist, &s->h_poll->sequence, s->poll_sequence, s->compute, s->d_alpha_ring, L.slots);
    } else {
        timed(&stats->time_reductions_ms, &stats->time_dot_rs_new_ms, [&] {
            launch_reduce_partials_and_step(s->partials_blas, cg_partial_count(nl), &s->d_s->rr_new, skip, s->compute, s->scratch(), s->d_s,
                                            config->tolerance, s->d_hist, &s->h_poll->sequence, s->poll_sequence, s->d_alpha_ring, L.slots, mailbox,
                                            &s->h_poll->progress, 4 * s->poll_sequence + 2);
        });
    }
    mark(enqueued, 5);
    ++enqueued;  // from here on `enqueued` is the number of the iteration just stepped (1-based), as the kernels count
}

void SolveRun::await_record(int iteration) {
    wait_for_record(s, sequence0 + iteration);
    if (iteration > records_read) records_read = iteration;
}

// Stage 5: p <- r + beta p and its halo exchange; nothing else before the host looks at the status: the GPU works on these
// while the host waits for the record. Late bulk: the piece the sweep walks first, then the status record, then -- unless the
// iteration converged -- the rest; the lead piece keeps the GPU busy while the host reads the record and launches.
void SolveRun::stage_direction_and_halo() {
    trace.push("BLAS_AXPBY");
    const size_t lo = L.bulk_lo, hi = L.bulk_hi;
    // the prediction is a local choice: any basis the host has will do
    const bool two_pieces = slab::two_pieces(L.late, lo, hi, s->lead_rows, s->late_predict && far_from_convergence(status(), records_read, enqueued, records_read));
    const Pieces piece = direction_pieces(lo, hi, s->lead_rows, backward, two_pieces);
    auto pieces = [&](auto&& first, auto&& rest) {
        timed(&stats->time_blas1_ms, &stats->time_axpby_update_p_ms, [&] {
            first(piece.first_lo, piece.first_rows);
            if (!two_pieces) return;
            s->enqueued_stage = "direction update (lead piece)";
            await_record(enqueued);
            if (!s->h_poll->converged) rest(piece.rest_lo, piece.rest_rows);  // else the loop ends here: nothing reads the rest of this direction
        });
    };
    if (L.slots == 1) {  // in-place form: x += alpha p rides with the direction update
        const double* x_in = enqueued == 1 ? s->x0 : s->x;
        auto px = [&](size_t off, size_t count) {
            if (count > 0) launch_cg_update_px(count, s->d_s, s->r + off, s->p + off, x_in + off, s->x + off, enqueued, s->compute, backward, s->device_form);
        };
        pieces(px, px);
    } else {
        // the slot the new direction goes to still holds p of iteration enqueued - slots: fold the whole window into x first
        // (alpha of this iteration is already on the stream: the step above wrote it)
        if (flush_due(enqueued, window_start, L.slots)) {
            timed(&stats->time_blas1_ms, nullptr, [&] {
                launch_cg_flush_x(nl, s->d_alpha_ring, flush_ring(), L.slots, window_start % L.slots, L.slots, flush_from(), s->x, s->compute,
                                  s->d_s, window_start);
            });
            window_start = enqueued;
        }
        double* p_next = s->ring[(size_t)(enqueued % L.slots)];
        const double* p_in = s->p;
        auto plain = [&](size_t off, size_t count) {
            if (count > 0) launch_cg_update_p_ring(count, s->d_s, s->r + off, p_in + off, p_next + off, enqueued, s->compute, backward, s->device_form);
        };
        auto fused = [&](size_t off, size_t count) {
            // the edge rows first (they raise the flag the exchange waits for), then this piece; the step too where it is due
            launch_cg_direction(DirectionLaunch{s->d_s, config->tolerance, enqueued, s->d_hist, step_in_direction ? &s->h_poll->sequence : nullptr,
                                                s->poll_sequence, s->d_alpha_ring, L.slots, s->r, p_in, p_next, off, count, backward, s->device_form},
                                &edges, s->scratch(), s->compute);
            s->p = p_next;  // the exchange sends from / receives into the new direction buffer
            trace.pop();
            {
                TraceScope r(trace, "Halo_Exchange");
                start_halo(s->p, /*released_by_flag=*/true);
            }
            trace.push("BLAS_AXPBY");
        };
        if (L.fused_direction) direction_from = p_in;  // no launch here: the next SpMV's launch evaluates r + beta p_in into p_next itself
        else if (L.pipeline) pieces(fused, plain);
        else pieces(plain, plain);
        s->p = p_next;
    }
    trace.pop();
    mark(enqueued - 1, 6);
    s->enqueued_stage = "direction update and halo exchange";
    if (!L.pipeline) {
        TraceScope r(trace, "Halo_Exchange");
        start_halo(s->p, /*released_by_flag=*/false);
    }
}

// The host reads the iteration's status record (the GPU is already busy with the direction update, the exchange and -- in the
// next turn of the loop -- the SpMV). Returns true when the loop is over.
bool SolveRun::read_status() {
    // The host may run ONE iteration ahead of the records it has seen (the three decisions are slab_decisions.hpp's):
    // while the residual it knows says the iteration just enqueued cannot be the converging one, it goes on to enqueue the next
    // iteration and reads the record on the way. The decision must be the SAME ON EVERY RANK (an iteration carries collectives):
    // it is taken from the residual history alone, never from whether a record happens to have arrived; and the verdict on an
    // iteration whose record was read late comes from the history too, not from the record's flag, which a later record may
    // already have overwritten. (A rank whose late bulk already told it the outcome follows the common rule too.)
    const int j = enqueued;
    if (catches_up(records_read, j)) {
        await_record(j - 1);
        if (ends_after_catch_up(status(), s->h_poll->converged != 0, j)) {  // the guess was wrong: iteration j was enqueued for nothing (its kernels saw the flag); the loop ends here
            await_record(j);
            return true;
        }
    }
    const bool deferred = defers_record(status(), s->run_ahead, config->verbose, records_read, j);
    if (!deferred) await_record(j);
    mailbox_check(s->comm);
    if (const int gave_up = __atomic_load_n(&s->h_poll->halo_late, __ATOMIC_ACQUIRE)) {
        if (s->selfcheck) {  // creation check: a hand-over that never came is a verdict, not the end of the process
            s->selfcheck_late = true;
            __atomic_store_n(&s->h_poll->halo_late, 0, __ATOMIC_RELEASE);
            return true;
        }
        // worded like the host watchdog's report: bench.py's supervisors read that sentence and restart the ranks once without the overlap
        fprintf(stderr, "\n[spmv_amd watchdog] rank %d: no progress for %.1f s in stage '%s' (CG iteration %d)\n", s->comm->rank, halo_wait_limit_s(s),
                gave_up == 3 ? "edge rows' ready flag (side-stream wait in front of the halo exchange)"
                             : "halo arrival flag (in-kernel wait of the boundary rows)",
                enqueued - 1);
        report_slab_state(s, stderr);
        exit(EXIT_FAILURE);
    }
    if (config->verbose >= 2 && s->comm->rank == 0) {
        CgScalars now;
        HIP_CHECK(hipMemcpy(&now, s->d_s, sizeof now, hipMemcpyDeviceToHost));
        if (s->label)  // cg_solve_device's line (reference cg_solver.cu:604-607)
            printf("[%s] Iter %3d: residual = %e (rel = %e)\n", s->label, now.iterations, now.residual, now.residual / now.b_norm);
        else
            printf("[Iter %3d] Residual: %.6e (rel: %.6e, alpha: %.4e)\n", now.iterations, now.residual, now.residual / now.b_norm, now.alpha);
    }
    // not deferred: record `enqueued` is the latest there can be (nothing of the next iteration is on the stream): its flag is exact
    return deferred ? false : s->h_poll->converged != 0;
}

// Averages over the counted iterations of a timeline solve; order = kTimelineNames.
void SolveRun::resolve_timeline(const CgScalars& fin, float total_ms) {
    auto us = [&](hipEvent_t a, hipEvent_t b) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        return (double)ms * 1e3;
    };
    const std::vector<hipEvent_t>& E = s->tl_compute;
    const size_t tl_flush = mark_index(enqueued, 0);  // [+0] before, [+1] after the final flush
    const int its = fin.iterations < enqueued ? fin.iterations : enqueued;
    // The direction update of the converging iteration does no work (its launch reads the flag and returns; with late
    // bulk only a lead piece is launched at all): it is left out of that stage's average, as the reference divides each
    // timer by the iterations that ran it (cg_solver_mgpu_partitioned.cu:770-800) and tests convergence before its p
    // update (:652-676). iteration_us stays the average over all counted iterations, the shorter last one included.
    const int direction_updates = fin.converged && its > 0 ? its - 1 : its;
    double stage[kTimelineMarks] = {0, 0, 0, 0, 0, 0, 0};  // [k] = mark k -> mark k+1; [6] = mark 6 -> next iteration's mark 0
    double iteration_us = 0.0;
    for (int it = 0; it < its; ++it) {
        const size_t base = mark_index(it, 0);
        for (int k = 0; k < kTimelineMarks - 1; ++k)
            if (k != 5 || it < direction_updates) stage[k] += us(E[base + k], E[base + k + 1]);
        const hipEvent_t next = it + 1 < enqueued ? E[base + kTimelineMarks] : E[tl_flush];  // the last counted iteration ends at the flush mark
        stage[6] += us(E[base + 6], next);
        iteration_us += us(E[base], next);
    }
    double side_us = 0.0;
    const int exchanges = tl_exchanges < its ? tl_exchanges : its;  // exchange j feeds the SpMV of iteration j
    for (int j = 0; j < exchanges; ++j) side_us += us(s->tl_side[2 * (size_t)j], s->tl_side[2 * (size_t)j + 1]);
    const double per = its > 0 ? 1.0 / its : 0.0;
    s->timeline_us = {(double)its, (double)total_ms, us(E[0], E[1]), stage[0] * per, stage[1] * per, stage[2] * per, stage[3] * per,
                      stage[4] * per, direction_updates > 0 ? stage[5] / direction_updates : 0.0, stage[6] * per, iteration_us * per,
                      exchanges > 0 ? side_us / exchanges : 0.0, us(E[tl_flush], E[tl_flush + 1]), (double)direction_updates};
    stats->time_spmv_ms = (s->timeline_us[3] + s->timeline_us[4]) * s->timeline_us[0] / 1e3;
}

// The last flush of x, the end of the timed region, and the outcome from what the scalar kernels left in host-coherent memory.
void SolveRun::finish() {
    s->shape.reverse = false;
    s->reduce_mailbox = nullptr;
    const size_t tl_flush = mark_index(enqueued, 0);
    if (timeline) HIP_CHECK(hipEventRecord(tl_event(s->tl_compute, tl_flush), s->compute));
    if (L.slots > 1 && enqueued > window_start)  // x <- x + the directions of the last window
        timed(&stats->time_blas1_ms, nullptr, [&] {
            launch_cg_flush_x(nl, s->d_alpha_ring, flush_ring(), L.slots, window_start % L.slots, enqueued - window_start, flush_from(), s->x, s->compute, s->d_s,
                              window_start);
        });
    s->p = s->ring[0];
    if (enqueued == 0)  // no iteration ran (max_iters == 0): the solution is the initial guess
        HIP_CHECK(hipMemcpyAsync(s->x, s->x0, nl * sizeof(double), hipMemcpyDeviceToDevice, s->compute));
    if (timeline) HIP_CHECK(hipEventRecord(tl_event(s->tl_compute, tl_flush + 1), s->compute));
    total.end(s->compute);
    float total_ms = 0.f;
    {
        WatchdogScope guard("draining the streams after the loop", s->comm->rank, enqueued, report_slab_state, s);
        total_ms = total.elapsed_ms();
        if (s->side) HIP_CHECK(hipStreamSynchronize(s->side));
    }
    HIP_CHECK(hipGetLastError());
    // Iteration count and flag from the last status record, ||r|| of the last counted iteration from the history -- which is
    // fin.residual when converged and sqrt(fin.rr_old) when not (the step moves rr_new into rr_old exactly then). Only a solve
    // longer than the history (2^20 iterations) has to fetch the device scalars.
    CgScalars fin;
    memset(&fin, 0, sizeof fin);
    if (enqueued > 0 && !s->op_failed) {
        fin.iterations = s->h_poll->iterations;
        fin.converged = s->h_poll->converged;
    }
    if (fin.iterations < s->hist_cap && !s->op_failed) {
        fin.residual = s->d_hist[fin.iterations];
        fin.rr_old = fin.residual * fin.residual;
    } else {
        HIP_CHECK(hipMemcpy(&fin, s->d_s, sizeof fin, hipMemcpyDeviceToHost));
    }
    if (timeline) {
        resolve_timeline(fin, total_ms);
    } else if (!L.detail) {  // timed SpMV launches that did real work (one per counted iteration), scaled to all of them
        double ms_sum = 0.0;
        s->last_spmv_each.clear();
        for (int k = 0; k < sampled; ++k) {
            if (sampled_iteration[k] >= fin.iterations) continue;
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, s->spmv_ev[2 * k], s->spmv_ev[2 * k + 1]));
            ms_sum += ms;
            s->last_spmv_each.push_back(ms);
        }
        stats->time_spmv_ms = s->last_spmv_each.empty() ? 0.0 : ms_sum / (double)s->last_spmv_each.size() * fin.iterations;
    }
    ++s->spmv_event_phase;
    s->last_spmv_ms = stats->time_spmv_ms;
    s->last_spmv_launches = fin.iterations;
    stats->iterations = fin.iterations;
    stats->converged = fin.converged;
    // not converged: the reference reports sqrt(rs_old) of the last completed iteration (:720-725)
    stats->residual_norm = (fin.converged || fin.iterations < s->hist_cap) ? fin.residual : sqrt(fin.rr_old);
    stats->time_total_ms = total_ms;
    if (!fin.converged && s->comm->rank == 0 && s->label == nullptr) printf("\nMax iterations reached without convergence\n");
    if (L.detail && stats->iterations > 0) {
        stats->time_dot_rs_new_ms /= stats->iterations;
        stats->time_axpy_update_r_ms /= stats->iterations;
        stats->time_axpby_update_p_ms /= stats->iterations;
    }
    const int count = fin.iterations + 1 < s->hist_cap ? fin.iterations + 1 : s->hist_cap;
    s->history.assign(s->d_hist, s->d_hist + count);
    last_cg_history() = s->history;
}

}  // namespace
}  // namespace slab
}  // namespace spmv_amd

extern "C" int spmv_amd_cg_slab_solve(SpmvAmdCgSlab* s, const CGConfigMultiGPU* config, CGStatsMultiGPU* stats) {
    SolveRun run(s, config, stats);
    // the reference's NVTX ranges (:540-717) as roctx ranges, when detailed timers (or SPMV_AMD_ROCTX=1) ask for them
    TraceScope solver_range(run.trace, "CG_Solver");
    run.begin();
    run.initial_residual();
    bool done = false;
    while (!done && !s->op_failed && run.enqueued < config->max_iters) {
        TraceScope iteration_range(run.trace, "CG_Iteration");
        run.stage_spmv();
        if (s->op_failed) break;  // nothing of this iteration is awaited yet
        run.stage_allreduce_pAp();
        run.stage_update_r();
        run.stage_sum_rr_and_step();
        run.stage_direction_and_halo();
        done = run.read_status();
    }
    run.finish();
    return s->op_failed ? 1 : 0;
}
