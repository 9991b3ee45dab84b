// cg_slab.hpp -- Conjugate Gradient on a 1-D row slab per GPU: the MI355X counterpart of reference
// src/solvers/cg_solver_mgpu_partitioned.cu:236-908 (the binary behind every published CG number, "1 GPU" included) and, through
// a slab that borrows the caller's SpmvOperator, of the single-GPU entry point cg_solve_device (cg_solver.cu:436-706).
// Same partition, local CSR, algebra, stopping rule and timed region; what is organised differently for the hardware, round by
// round, is DESIGN §4. This header: the slab record and what the pieces share. The pieces (host code only, no kernel):
//   slab_decisions.hpp    every decision that is a pure function of integers and doubles (no HIP; tests/abi/slab_decisions_test.cpp)
//   cg_slab_create.hip    creation and destruction: streams, arena, ring, planes, tile classes, placement and tile-run trials, creation check
//   cg_slab_solve.hip     one solve: the slab's SpMV forms, the waits and the exchange, SolveRun's stages, spmv_amd_cg_slab_solve
//   cg_slab_api.hip       accessors, the LAB build's options and single stages, time_spmv
//   cg_device.hip         cg_solve_device's workspace and the reference-named entry points (cg_solve_on_operator, cg_solve_mgpu_partitioned)
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "comm.hpp"
#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "skew_geometry.hpp"
#include "slab_decisions.hpp"
#include "solve_common.hpp"
#include "stencil_geometry.hpp"
#include "trace_ranges.hpp"
#include "watchdog.hpp"

using namespace spmv_amd;

struct SpmvAmdCgSlab {
    SpmvAmdComm* comm = nullptr;
    // Which slab of how many this is. Equal to the communicator's rank / world, except for a stand-in slab
    // (spmv_amd_cg_slab_create_stencil5_as): one self-neighbour rank carrying the slab of rank `part_rank` of a
    // `part_world`-GPU job, so that one GPU can time the real per-rank slab shapes.
    int part_rank = 0, part_world = 1;
    // Borrowed operator (cg_solve_device, reference src/solvers/cg_solver.cu:436-706): the matrix stays with the caller's
    // SpmvOperator and every SpMV goes through its vtable's run_device -- or, when the operator is this library's own
    // stencil5-csr, through its fused launch (FusedSpmv: p.Ap partials / initial residual written by the SpMV itself).
    // Such a slab is the whole matrix on one rank, has no halos, and runs on the DEFAULT stream, where run_device enqueues.
    SpmvOperator* op = nullptr;
    bool op_failed = false;  // the borrowed operator's run_device returned non-zero: the solve stops enqueuing and returns 1
    FusedSpmv fused;
    const char* label = nullptr;  // verbose prefix of the reference entry point that owns the solve ("CG-DEVICE")
    bool device_form = false;     // direction update rounded as update_p_kernel does (cg_solver.cu:90-95), see cg_kernels.hip
    int n = 0, grid = -1, row_offset = 0, n_local = 0, halo = 0;
    bool has_prev = false, has_next = false;
    slab::RowRange halo_free() const { return slab::halo_free_rows(n_local, halo, has_prev, has_next); }  // the rows that need no halo
    DeviceCsr A;
    double *x = nullptr, *x0 = nullptr, *r = nullptr, *Ap = nullptr, *b = nullptr;
    double* x0_alloc = nullptr;  // x0 carries halo rows too ([pad | prev halo | local | next halo]): the initial SpMV reads it in place
    // Vector arena: r, Ap and every direction buffer are carved out of ONE allocation, in that order (kernels that walk vectors in
    // lock step lose 6.5 % when the vectors lie in different classes of 32 GiB address regions). The SpMV's coefficient
    // stream does not take part (place_coefficients).
    double* vec_arena = nullptr;
    // Symmetric coefficient form (kernels.hpp, SymPlanes): [C, E] and S planes (S with one grid row of halo) in ONE allocation
    // next to the CSR, streamed by the row-lds launches: 24 B/row instead of 40. The CSR stays for the grid's first and last grid row.
    double* planes_alloc = nullptr;
    size_t planes_doubles = 0, planes_s_offset = 0;  // the allocation's length; where the S plane's local part starts
    SymPlanes planes;
    bool planes_on = false;
    // Tile classes (kernels.hpp, SymPlanes; classify_tiles): one byte per row-lds tile, 1 where every coefficient the tile multiplies
    // equals the slab-wide quintuple bit for bit -- such a tile loads none. Written once at creation; the planes stay allocated.
    unsigned char* tile_classes = nullptr;
    size_t tile_class_count = 0;                  // local grid rows x tiles per grid row
    long long tiles_uniform = 0, tiles_total = 0; // of the tiles of the grid rows that are evaluated from the planes
    double quintuple[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // W, C, E, N, S
    bool stream_everywhere = false;  // LAB option: the kernel ignores the map and streams the planes on every tile
    // Block maps (kernels.hpp, Stencil5Plan::block_map; build_block_maps), derived from tile_classes: one per launch range of the
    // in-loop SpMV -- the ranges start at different grid rows, so their blocks of knobs.rowlds_block_rows grid rows hold different rows.
    unsigned char *block_map_whole = nullptr, *block_map_interior = nullptr;
    // The blocks of each range whose map byte is 0, in ascending order (device memory; the counts stay on the host): the launch that
    // follows the direction update inside the block SpMV evaluates exactly these (kernels.hpp, DirectionSpmv).
    int *slow_list_whole = nullptr, *slow_list_interior = nullptr;
    int slow_count_whole = 0, slow_count_interior = 0;
    // SPMV_AMD_FUSED_DIRECTION (0 / 1, read at creation): the direction update inside the block SpMV where the slab is eligible
    // (LoopShape::fused_direction). LAB build, set_option("fused_direction", 2): on regardless of the slow blocks' share.
    int fused_direction = 1;
    // SPMV_AMD_AP_RECOMPUTE (0 / 1, read at creation; LAB build: set_option("ap_recompute", 0 | 1)): on top of the fused direction
    // update, A p' is not stored on the fast blocks and the r update recomputes it from p' (LoopShape::ap_recomputed).
    // row_block_fast (device, with the block maps): one byte per row block of the whole-slab map, 1 = every block tile is fast;
    // skew_eligible: no row block is mixed (skew_geometry.hpp). last_*: what the last solve did (LAB hook spmv_amd_cg_slab_ap_form).
    int ap_recompute = 1;
    unsigned char* row_block_fast = nullptr;
    bool skew_eligible = false;
    bool last_ap_recomputed = false;
    int last_recompute_launches = 0;
    // SPMV_AMD_FIRST_RECOMPUTE (0 / 1, read at creation; LAB build: set_option("first_recompute", 0 | 1)): iteration 0 takes the same
    // form (LoopShape::first_recomputed, slab_decisions.hpp first_form). last_first_form: what the last solve's iteration 0 took, as
    // a FirstForm; counted apart from last_recompute_launches, which keeps meaning the launches of iterations >= 1.
    int first_recompute = 1;
    int last_first_form = 0;
    // x0 holds the zeros the LIBRARY wrote (the fill at creation, the API's default initial guess) and nothing has written it since:
    // every other writer of x0 clears this, an uploaded vector of zeros included -- x0 is never scanned. What it buys: DESIGN §4,
    // LoopShape::zero_start (the first launch) and flush_skips_x0 (every slab: the flush is pointwise).
    bool x0_known_zero = false;
    // SPMV_AMD_ZERO_START (0 / 1, read at creation; LAB build: set_option("zero_start", 0 | 1)): 0 = x0 is always loaded and the first
    // launch stores r0 twice, the launches of before.
    bool zero_start = true;
#ifdef SPMV_AMD_LAB
    // set_option("zero_start_parts", mask), for A/B runs of each part: 1 = first launch without x loads, 2 = r0 stored once, 4 = flush without x_in,
    // 8 = b serves as p0 and iteration 0's SpMV sums b.b (LoopShape::b_is_p0)
    int zero_start_parts = 15;
#else
    static constexpr int zero_start_parts = 15;
#endif
    int zero_start_mask() const { return zero_start ? zero_start_parts : 0; }  // slab_decisions.hpp, ShapeInputs::zero_start_parts
    // A 0 is +0.0 on every local row (slab_decisions.hpp, sums_to_plus_zero; one pass over the CSR values at creation, next to the class
    // map; slabs that keep the planes only). No entry point rewrites a slab's coefficients after creation -- the placement trial
    // copies them bit for bit -- so nothing clears it. partials_first: the b.b partials of LoopShape::b_is_p0's first launch, one per
    // slot of the whole-slab plan (partials_blas is shorter than that, and partials_spmv takes the launch's p.Ap partials).
    bool zero_rows_plus_zero = false;
    double* partials_first = nullptr;
    bool spmv_with_dot = false;  // LAB option: spmv_amd_cg_slab_spmv runs the in-loop form (dot partials wanted)
    const SymPlanes* sym() const { return planes_on ? &planes : nullptr; }
    // place_coefficients: {0, candidates timed, SpMV ms before, SpMV ms kept}
    std::vector<double> placement;
    std::vector<double> tile_runs;  // tune_tile_runs: {rule, kept, SpMV ms with the rule, ms kept}; empty = did not run
    // wall ms of the set-up phases of creation, each closed by a device synchronisation (spmv_amd_cg_slab_setup_ms):
    // matrix to HBM (upload or generation), streams + vectors, verification + launch plans, coefficient placement, tile runs
    double setup_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // false for the slab a one-shot entry point creates, solves on once and destroys (cg_solve_mgpu_partitioned): the two timed
    // trials of creation cost 0.05-5 s and can win back 2 % of ONE solve at most
    bool setup_trials = true;
    double* p_alloc = nullptr;  // [pad | prev halo | local | next halo]
    double* p = nullptr;        // local part of the CURRENT direction vector, 16-byte aligned
    // Direction ring (deferred x update): with ring_slots > 1 the direction update is written out of place into the next
    // of ring_slots halo-carrying buffers and x = x0 + sum alpha_k p_k is evaluated by one flush pass per ring_slots iterations
    // (and at the end), same fma chain per element in the same order; ring_slots = 1 is the in-place form.
    size_t slot_doubles = 0, slot_lead = 0;  // size of one halo-carrying buffer and where its local part starts
    std::vector<double*> ring_alloc;  // allocations, ring_alloc[0] == p_alloc
    std::vector<double*> ring;        // local parts
    int ring_slots = 1;
    double* d_alpha_ring = nullptr;
    double* partials_spmv = nullptr;  // dot partials of the SpMV launches (interior, head, tail back to back)
    double* partials_blas = nullptr;
    double* reduce_stage = nullptr;  // scratch of this slab's reductions (kernels.hpp, ReduceScratch)
    // One launch per dot product (round 5, reduce_device.hpp); the boundary rows of a split SpMV ride in the launch that
    // reduces the SpMV's partials (launch_stencil5_edges_and_reduce).
    ReduceScratch scratch() const { return ReduceScratch{reduce_stage}; }
    CgScalars* d_s = nullptr;
    double* d_hist = nullptr;
    int hist_cap = 0;
    // pinned, host-coherent. progress = 4 * sequence + k, written by the last block of the local reductions of the
    // iteration that will publish `sequence`: k = 1 local p.Ap summed, k = 2 local r.r summed (watchdog report only)
    // halo_late: set by a boundary wave that gave up waiting for the halo's arrival flag (kernels.hpp, HaloArrival)
    struct Poll { int sequence; int converged; int iterations; int progress; int halo_late; }* h_poll = nullptr;
    // Device-side arrival flag of the halo exchange: behind every exchange on the SIDE stream a one-thread launch raises
    // *d_halo_flag to that exchange's sequence number, and the boundary waves of the launch that needs the halo rows wait for it
    // themselves -- no cross-stream event wait between a SpMV and its dot product.
    unsigned* d_halo_flag = nullptr;
    unsigned halo_sequence = 0;
#ifdef SPMV_AMD_LAB
    // Measurement hook, set_option("stop_at", k): iteration k counts as the converging one whatever its residual (CgScalars::stop_at):
    // a stand-in slab's mirrored system does not converge in 14 iterations as the rank of a real job does. Timing only.
    int stop_at = 0;
    int test_wedge_overlapped_exchange = 0;  // SPMV_AMD_TEST_WEDGE_OVERLAPPED_EXCHANGE=1 / 2, see exchange_halo
    bool lab_first_store = true;  // set_option("first_store", 0): spmv_amd_cg_slab_first_stage runs the launch that does not store A b
    bool lab_direction_store = true;  // set_option("direction_store", 0): spmv_amd_cg_slab_direction_spmv runs the launch that does not store A p'
    bool guess_far_always = false;  // set_option("run_ahead", 2): every iteration is guessed "cannot converge": each solve learns of its convergence one iteration late
#endif
    // non-null while a solve runs on a communicator with a working peer mailbox: the last stage of every dot
    // product then completes the sum across the ranks itself (no all-reduce launch)
    const PeerMailbox* reduce_mailbox = nullptr;
    int* spmv_progress = nullptr;  // where the p.Ap reduction of the SpMV being enqueued reports (in-loop SpMVs only)
    int spmv_progress_value = 0;
    const char* enqueued_stage = "";  // the last piece of work the host put on the streams
    int enqueued_iteration = -1;
    hipStream_t compute = nullptr, side = nullptr;
    bool owns_streams = true;
    hipEvent_t ev_p_ready = nullptr, ev_halo_done = nullptr;
    // Timeline of a solve (spmv_amd_cg_slab_set_timeline): events at the stage boundaries of every iteration, recorded
    // without any host sync and resolved after the loop. kTimelineMarks per iteration on the compute stream, two on the
    // side stream around the halo exchange.
    bool timeline_on = false;
    std::vector<hipEvent_t> tl_compute, tl_side;
    hipEvent_t tl_after_interior = nullptr;  // where slab_spmv marks the end of the interior launch (split SpMV)
    std::vector<double> timeline_us;         // result of the last timeline solve, order = kTimelineNames
    LaunchShape shape;
    // launch plans, made once at creation: the whole slab, the rows that need no halo, the first / last grid row
    Stencil5Plan plan_whole, plan_interior, plan_head, plan_tail;
    int partials_cap = 0;
    int spmv_split_at = -1;  // set by slab_spmv: partials written by the interior launch of a split SpMV (-1: one launch)
    const char* variant_name = "";
    bool fused_dot = false;
    bool fuse_init_residual = false;  // r0 = b - A x0, p0, r0.r0 written by the first SpMV's launches (row-lds slabs)
    std::vector<double> history;
    // event pairs around every spmv_event_stride-th in-loop SpMV (no host sync, resolved after the loop): time_spmv_ms with timers
    // off is the live average of those launches times the iteration count. A pair costs two barrier packets (~7 us each), so every
    // 7th launch is timed and the phase moves on by one with every solve. (LAB build: set_option("spmv_event_stride", 1 | 0).)
    std::vector<hipEvent_t> spmv_ev;
    int spmv_event_stride = 7;
    int spmv_event_phase = 0;  // solves so far
    bool roctx_always = false;  // SPMV_AMD_ROCTX=1: roctx ranges even without detailed timers
    bool no_overlap = false;  // SPMV_AMD_NO_OVERLAP=1: the PLAIN loop shape (halo exchange on the compute stream: the reference's; bench.py's fallback)
    // verify_pipeline's two short solves: waits on the other stream's flags give up after wait_limit_s instead of 20 s, and a
    // wait that gave up ends that solve (selfcheck_late) instead of the process
    bool selfcheck = false, selfcheck_late = false;
    double wait_limit_s = 0.0;  // 0 = the default bound (halo_wait_limit_s)
    // Late bulk (slabs of >= 1e8 rows, ring mode): the direction update is enqueued as a LEAD piece of lead_rows rows,
    // then the host reads the status record and enqueues the rest only if the loop goes on -- the converging iteration no longer
    // dispatches 3 M workgroups that only read a flag. Same kernel over disjoint row ranges: same bits.
    bool late_bulk = false;
    // ... and only in iterations that MAY converge, judged by the residual the host already knows (slab_decisions.hpp,
    // far_from_convergence). (LAB build: set_option("late_bulk", 1) forces the protocol in every iteration.)
    bool late_predict = true;
    // The host runs one iteration ahead of the status records while convergence is far (SolveRun::read_status): an iteration's
    // worth of work is always queued, so a host that answers late does not idle the GPU. (LAB build: set_option("run_ahead", 0).)
    bool run_ahead = true;
    // 2^25 rows = ~125 us of streaming against ~20 us of host read + launch; 2^22 ... 2^26 all within 0.1 % (profiles/r06_ab_lead_rows.txt)
    size_t lead_rows = (size_t)1 << 25;
    int poll_sequence = 0;
    double last_spmv_ms = 0.0;
    int last_spmv_launches = 0;
    std::vector<float> last_spmv_each;  // the timed in-loop launches of the last solve, in iteration order
};

// marks per iteration on the compute stream: iteration start | interior SpMV enqueued-and-done | boundary rows |
// p.Ap sum (+ all-reduce) | r update | r.r sum (+ all-reduce) + scalar step | direction update
// (LoopShape::fused_direction: the direction update rides in the next iteration's SpMV launch, so spmv_interior_us of iterations
// >= 1 is that launch -- direction update, SpMV and the launch over the slow blocks -- and direction_update_us holds no launch: it
// reports what lies between its two marks, the event records themselves (a few us; and a window flush where the ring is shorter
// than the solve), so that the stages still add up to the iteration; direction_updates is counted as before)
constexpr int kTimelineMarks = 7;
constexpr const char* kTimelineNames =
    "iterations,solve_ms,initial_residual_us,spmv_interior_us,halo_wait_and_boundary_rows_us,reduce_pAp_and_allreduce_us,"
    "update_r_us,reduce_rr_allreduce_and_scalar_step_us,direction_update_us,gap_before_next_iteration_us,iteration_us,"
    "halo_exchange_on_side_stream_us,final_x_flush_us,direction_updates";

// ---- what the pieces share (internal linkage ends at the library's export map) ----
namespace spmv_amd {
std::vector<double>& last_cg_history();
#ifdef SPMV_AMD_LAB
const SpmvAmdCgSlab* cg_workspace_slab();  // cg_device.hip
#endif
namespace slab {
// cg_slab_create.hip
void adopt_operator(SpmvAmdCgSlab* s, SpmvOperator* op);
void make_common(SpmvAmdCgSlab* s);
SpmvAmdCgSlab* create_from_matrix(MatrixData* mat, SpmvAmdComm* comm, bool setup_trials);
SymPlanes plane_view(const SpmvAmdCgSlab* s, const double* base);
void build_block_maps(SpmvAmdCgSlab* s);
void poison_halos(SpmvAmdCgSlab* s);
// cg_slab_solve.hip
ShapeInputs shape_inputs(const SpmvAmdCgSlab* s, bool detailed_timers);
inline LoopShape loop_shape(const SpmvAmdCgSlab* s, bool detailed_timers = false) { return loop_shape(shape_inputs(s, detailed_timers)); }
int slab_spmv(SpmvAmdCgSlab* s, bool with_dot, bool overlap, const int* skip, const double* input = nullptr, hipEvent_t spmv_done = nullptr,
              const ResidualOut* init = nullptr, bool x_zero = false, bool ap_not_stored = false);
int slab_direction_spmv(SpmvAmdCgSlab* s, const double* p_in, double* p_out, int iteration, hipEvent_t spmv_done = nullptr, bool ap_not_stored = false);
int slab_update_r_recompute(SpmvAmdCgSlab* s, const double* p_new, bool reverse, bool r_is_p = false);
int slab_initial_residual(SpmvAmdCgSlab* s, const LoopShape& L, bool halo_in_flight);
int slab_first_spmv(SpmvAmdCgSlab* s, bool reverse, hipEvent_t spmv_done = nullptr, bool ap_not_stored = false);
void reduce_spmv_partials(SpmvAmdCgSlab* s, int used, double* d_out, const int* skip, int* progress, int progress_value, const PeerMailbox* mailbox,
                          const double* partials = nullptr);
void report_slab_state(void* user, FILE* out);
}  // namespace slab
}  // namespace spmv_amd
using namespace spmv_amd::slab;
