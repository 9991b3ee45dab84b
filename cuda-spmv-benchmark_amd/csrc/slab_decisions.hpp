// slab_decisions.hpp -- every decision of the CG slab solver that is a pure function of a few integers and doubles: which shape a
// solve's loop takes, when the host may run ahead of the status records, where the direction update is cut, how the buffers are
// laid out and how long the direction ring gets. Standard headers only: no HIP, no SpmvAmdCgSlab, nothing here prints, allocates
// or reads the environment, so tests/abi/slab_decisions_test.cpp calls all of it on a CPU. The callers (cg_slab_create.hip,
// cg_slab_solve.hip, cg_slab_api.hip) keep the waiting, the launching and the printing. Why each rule is what it is: DESIGN §4.
#ifndef SPMV_AMD_SLAB_DECISIONS_HPP
#define SPMV_AMD_SLAB_DECISIONS_HPP
#include <cstddef>

namespace spmv_amd {
namespace slab {

// ---- layout ----
// 4 KiB = 512 doubles: the local part of every halo-carrying buffer, the S plane's local part and the launch ranges of the direction
// update start on such a boundary (a halo of 14 142 doubles put every access across two 128-byte lines; line-aligned but not
// 4 KiB-aligned parts still cost 4-8 % in the streaming kernels).
constexpr size_t kUnit = 512;
inline size_t round_up(size_t doubles) { return (doubles + kUnit - 1) / kUnit * kUnit; }
inline size_t round_down(size_t doubles) { return doubles / kUnit * kUnit; }

// Which sides of the slab have a neighbour, and the halo length. A self-neighbour rank that owns the WHOLE grid (part_world == 1)
// keeps halos on both sides: the rows that would read them are the global grid's first and last grid row, which have no north /
// south entry, so the full pipeline runs and the solve must still reproduce the plain one (tests/test_distributed.py).
struct Sides { bool has_prev, has_next; int halo; };
inline Sides slab_sides(bool exchanges_halos, int part_rank, int part_world, bool self_neighbour, int grid) {
    const bool whole_grid_probe = self_neighbour && part_world == 1;
    return Sides{exchanges_halos && (part_rank > 0 || whole_grid_probe), exchanges_halos && (part_rank < part_world - 1 || whole_grid_probe),
                 exchanges_halos ? grid : 0};
}

// The rows [lo, hi) of the slab whose north and south neighbours are local: they need no halo.
struct RowRange { int lo, hi; };
inline RowRange halo_free_rows(int n_local, int halo, bool has_prev, bool has_next) {
    return RowRange{has_prev ? halo : 0, n_local - (has_next ? halo : 0)};
}

// One halo-carrying buffer [pad | prev halo | local | next halo] and the arena that holds r, Ap and the ring: `lead` doubles in
// front of the local part, one vector every `pitch` doubles -- the vector rounded up to 2 MiB, plus 4 KiB, so that consecutive
// vectors differ in their phase inside the memory system's interleave as well (profiles/r04_arena_probe.txt).
struct SlotLayout { size_t lead, slot_doubles, pitch; };
inline SlotLayout slot_layout(size_t n_local, int halo) {
    constexpr size_t k2MiB = (size_t)2 << 20, k4KiB = 4096;
    SlotLayout l;
    l.lead = round_up((size_t)halo);
    l.slot_doubles = l.lead + n_local + (size_t)halo + 2;
    l.pitch = ((l.slot_doubles * sizeof(double) + k2MiB - 1) / k2MiB * k2MiB + k4KiB) / sizeof(double);
    return l;
}

// The symmetric planes in ONE allocation: [C, E] first, then the S plane with one grid row of halo, its local part on a 4 KiB boundary.
struct PlaneLayout { size_t ce, halo_lead, total, s_offset; };
inline PlaneLayout plane_layout(size_t n_local, int grid) {
    PlaneLayout l;
    l.ce = round_up(2 * n_local);
    l.halo_lead = round_up((size_t)grid);
    l.total = l.ce + l.halo_lead + n_local;
    l.s_offset = l.ce + l.halo_lead;
    return l;
}

// A slab whose launches can all be row-lds launches (whole grid rows of a grid that takes row-lds) and that owns its matrix: worth
// reserving the planes for before the ring takes what is free.
inline bool may_take_planes(bool owns_matrix, int grid, int rowlds_min_grid, int n_local, int row_offset) {
    return owns_matrix && grid >= 2 && grid >= rowlds_min_grid && n_local > 0 && n_local % grid == 0 && row_offset % grid == 0;
}

constexpr size_t kKeepFree = (size_t)4 << 30;  // left to the caller's own buffers
// The planes are taken where r, Ap, the first direction buffer and a ring of 4 still fit beside them. per_slot = pitch in bytes.
inline bool planes_fit(size_t free_bytes, size_t plane_bytes, size_t per_slot) { return free_bytes > plane_bytes + kKeepFree + 3 * per_slot + 3 * per_slot; }

// The direction ring's length: what was asked (SPMV_AMD_P_RING; the default is max_slots), held to 1..max_slots and to the
// memory. A slab that owns its matrix may take what is free beyond kKeepFree and r, Ap and the first buffer; the workspace of
// cg_solve_device outlives the call next to a caller who goes on allocating, so it is held to a quarter of what is free now.
// A ring cut short by memory to fewer than 4 flushes too often to pay: it becomes the in-place form.
inline int ring_length(int asked, size_t per_slot, size_t free_bytes, bool borrowed_operator, int max_slots) {
    const int clamped = asked < 1 ? 1 : (asked > max_slots ? max_slots : asked);
    const size_t fixed = 3 * per_slot;
    const size_t budget = borrowed_operator ? free_bytes / 4 : (free_bytes > kKeepFree + fixed ? free_bytes - kKeepFree - fixed : 0);
    int want = clamped;
    while (want > 1 && (size_t)(want - 1) * per_slot > budget) --want;
    return want < clamped && want < 4 ? 1 : want;
}

enum class Partition { Ok, NeedsStencil, ThinnerThanGridRow };
inline Partition partition_check(bool exchanges_halos, int grid, int n_local) {
    if (!exchanges_halos) return Partition::Ok;
    if (grid <= 0) return Partition::NeedsStencil;
    return n_local < grid ? Partition::ThinnerThanGridRow : Partition::Ok;
}

inline bool late_bulk_default(size_t n_local) { return n_local >= 100000000; }
// Grid rows per block tile of a slab's in-loop SpMV (Tunables::rowlds_block_rows) where nobody asked (asked < 0; SPMV_AMD_ROWLDS_BLOCK_ROWS
// of 0, 4 or 8 is taken as it is, any other value counts as not asked): 8 where the loop can take the direction update inside the block SpMV -- a slab
// without neighbours that owns its matrix, with a direction ring, fused_direction not switched off -- which ran ahead of 4 every time
// both were measured there; 4 for every other slab: the plain block kernel measured faster with 4, and nothing between
// devices has been measured with 8.
inline int default_block_rows(int asked, bool exchanges_halos, bool owns_matrix, int ring_slots, int fused_direction) {
    if (asked == 0 || asked == 4 || asked == 8) return asked;
    return !exchanges_halos && owns_matrix && ring_slots > 1 && fused_direction != 0 ? 8 : 4;
}
// the coefficient placement trial: slabs of >= 16 Mi rows, where the device offers more than one candidate region
inline bool wants_coefficient_placement(size_t n_local, int candidates) { return n_local >= ((size_t)16 << 20) && candidates > 1; }
// In-kernel / side-stream waits for the other stream's flags give up well inside the host's watchdog (limit 0 = none set).
inline double halo_wait_limit_s(double override_s, double watchdog_s) {
    if (override_s > 0.0) return override_s;
    return watchdog_s > 0.0 && watchdog_s < 40.0 ? 0.5 * watchdog_s : 20.0;
}
// residual history: one slot per iteration and one for ||r0||, capped at 2^20 entries (later iterations go unrecorded)
inline int want_hist(int max_iters) { return max_iters < (1 << 20) ? max_iters + 1 : (1 << 20); }

// slab_spmv: the boundary rows of a split in-loop SpMV ride in the launch that reduces the partials where they are whole grid
// rows, at most one per side. head_rows / tail_rows = the rows in front of / behind the halo-free range.
inline bool fused_tail(bool with_dot, bool writes_partials, bool initial_residual, int head_rows, int tail_rows, int grid) {
    return with_dot && writes_partials && !initial_residual && head_rows % grid == 0 && tail_rows % grid == 0 && head_rows <= grid && tail_rows <= grid;
}

// ---- a fact about the matrix, established once at creation ----
// Does a row with these stored coefficients sum to +0.0, bit for bit, when every operand is +0.0 -- in whatever order the products
// are added, started from 0.0 or from the first product (the interior fma chain, the CSR loop on edge columns and on the grid's
// first and last grid row)? Every product of a finite coefficient and +0.0 is a zero with the coefficient's sign, and a sum of
// zeros is -0.0 only if every addend is: so it is enough that every coefficient is finite and one has its sign bit clear. An
// infinity or a NaN gives NaN. Conservative (a chain started from 0.0 gives +0.0 for all-negative rows too) and order-independent.
// constexpr: the creation pass evaluates the same function on the GPU (spmv_kernels.hip, rows_plus_zero_kernel).
constexpr bool finite_value(double v) { return __builtin_isfinite(v); }
constexpr bool sign_bit_clear(double v) { return !__builtin_signbit(v); }
constexpr bool sums_to_plus_zero(const double* coefficients, int count) {
    bool finite = true, some_plus = false;
    for (int k = 0; k < count; ++k) {
        finite = finite && finite_value(coefficients[k]);
        some_plus = some_plus || sign_bit_clear(coefficients[k]);
    }
    return finite && some_plus;
}

// ---- the loop's shape, chosen once per solve ----
struct ShapeInputs {
    bool exchanges_halos, collective, mailbox_ready;  // the communicator's answers
    bool detailed_timers;
    int ring_slots;
    size_t n_local;
    int halo;
    bool has_prev, has_next;
    bool owns_matrix;     // op == nullptr
    bool no_overlap;
    bool reduce_scratch;  // the reductions' scratch is there
    int fused_direction;  // the option: 0 off, 1 where eligible, 2 whatever the slow blocks' share
    // what the direction update inside the block SpMV needs of the whole-slab launch
    bool fused_dot, planes_and_classes, block_plan;  // block_plan: row-lds with block rows and a block map
    int slow_blocks;                                 // < 0: they could not be listed
    long long block_tiles;
    bool late_bulk, fuse_init_residual, x0_known_zero;
    // 0 with zero_start off; else 1 = first launch without x loads, 2 = r0 stored once, 4 = flush without x_in, 8 = b serves as p0
    int zero_start_parts;
    bool zero_rows_plus_zero;  // established at creation: every row of A sums to +0.0 over zero operands (sums_to_plus_zero)
    // the r update that recomputes A p' (skew_geometry.hpp): the option (0 off, 1 where eligible) and whether every row block of the
    // whole-slab launch's block map is all-fast or all-slow (skew_eligible, established with the block maps)
    int ap_recompute;
    bool skew_eligible;
    int first_recompute;  // the option (0 off, 1 where ap_recomputed holds): iteration 0 in the same store-less form
};

struct LoopShape {
    bool multi = false;        // halo exchange needed
    bool reduce = false;       // all-reduce of the dot products needed
    bool separate = false;     // ... as a call of its own (RCCL / staged); false: inside the sums' last stage (peer mailbox) or not at all
    bool use_mailbox = false;  // the communicator's peer mailbox completes the sums
    bool detail = false;       // the reference's per-category timers: a host sync per stage, everything on the compute stream
    // PIPELINE: the exchange on the side stream under the interior rows, the boundary rows behind its arrival flag, and the rows
    // the neighbours wait for + the first piece of the rest + (RCCL path) the scalar step in ONE direction launch whose device
    // flag releases the exchange. false = PLAIN: everything on the compute stream, the exchange behind the whole direction update.
    bool pipeline = false;
    bool late = false;  // direction update as lead piece + rest (late bulk)
    // The direction update of iteration k rides in the SpMV launch of iteration k + 1: a slab without neighbours that owns its
    // matrix, the direction ring, no detailed timers, a whole-slab plan on the block kernel whose slow blocks are at most 1 / 16 of
    // its blocks. The direction stage then enqueues no vector launch and late bulk has nothing to split.
    bool fused_direction = false;
    // On top of fused_direction, in iterations >= 1: the fused launch does not store A p' on its fast blocks and the r update
    // recomputes it from p' on skewed block tiles (skew_geometry.hpp; cg_update_r_recompute_kernel): 16 B/row less per iteration.
    // Iteration 0 and every slab that is not eligible keep the stored A p and cg_update_r_kernel.
    bool ap_recomputed = false;
    // On top of ap_recomputed, in iteration 0: the SpMV of that iteration (the first launch on b, or the block kernel on p0) does not
    // store A p0 on its fast blocks either, and the r update recomputes it from the ONE vector that is both r0 and p0 there
    // (first_form below says which): 14 B/row less, once per solve.
    bool first_recomputed = false;
    // The two ends of a solve on a slab without neighbours that owns its matrix and takes the initial residual from the first
    // SpMV's launch. zero_start: x0 holds the library's own zeros, and that launch requests no x value on interior grid rows.
    // r0_in_ring (any x0): the launch stores r0 once, as p0 into ring slot 0, and the r update of iteration 0 reads it there.
    bool zero_start = false, r0_in_ring = false;
    // On top of both, where A 0 is +0.0 on every row (ShapeInputs::zero_rows_plus_zero): r0 = b - A 0 is b bit for bit, so nothing
    // computes or stores it. The first launch of the solve is iteration 0's block SpMV on b, which also sums b.b; b is read wherever
    // the first window reads ring slot 0, and is never written. Needs the block kernel on the whole slab and no detailed timers.
    bool b_is_p0 = false;
    int slots = 1;  // direction ring length; 1 = the in-place x / p update
    // pipeline: the edge ranges [0, head_rows) and [tail_start, n_local), rounded OUTWARDS to 4 KiB; the other rows are the bulk
    size_t head_rows = 0, tail_start = 0;
    size_t bulk_lo = 0, bulk_hi = 0;
};

// Can the whole-slab launch take the direction update inside the block SpMV? cap: the slow blocks are at most 1 / 16 of the
// range's blocks -- each of them costs a second pass over its rows, so a matrix with few uniform tiles keeps the two launches.
inline bool direction_spmv_available(const ShapeInputs& in, bool cap) {
    if (!in.owns_matrix || !in.fused_dot || !in.planes_and_classes || !in.block_plan || in.slow_blocks < 0) return false;
    return !cap || 16LL * in.slow_blocks <= in.block_tiles;
}

inline LoopShape loop_shape(const ShapeInputs& in) {
    LoopShape L;
    const size_t nl = in.n_local;
    L.multi = in.exchanges_halos;
    L.reduce = in.collective;
    L.use_mailbox = L.reduce && in.mailbox_ready;
    L.separate = L.reduce && !L.use_mailbox;
    L.detail = in.detailed_timers;
    L.slots = in.ring_slots;
    // (ring mode only: with the in-place form the x update of the converging iteration rides in that very launch)
    L.fused_direction = in.fused_direction != 0 && !L.multi && in.owns_matrix && L.slots > 1 && !L.detail &&
                        direction_spmv_available(in, /*cap=*/in.fused_direction != 2);
    L.ap_recomputed = L.fused_direction && in.ap_recompute != 0 && in.skew_eligible;
    L.first_recomputed = L.ap_recomputed && in.first_recompute != 0;
    L.late = in.late_bulk && !L.detail && L.slots > 1 && !L.fused_direction;
    // (ring mode only, like fused_direction: the in-place form keeps every launch it had)
    const bool own_ends = !L.multi && in.owns_matrix && L.slots > 1 && in.fuse_init_residual;
    L.zero_start = own_ends && in.x0_known_zero && (in.zero_start_parts & 1) != 0;
    L.r0_in_ring = own_ends && (in.zero_start_parts & 2) != 0;
    L.b_is_p0 = L.zero_start && L.r0_in_ring && in.zero_rows_plus_zero && in.fused_dot && in.planes_and_classes && in.block_plan && !L.detail &&
                (in.zero_start_parts & 8) != 0;
    // Early halo: the two edge ranges are rounded outwards, so that the launch over the rest starts on a 4 KiB boundary like every
    // whole-vector launch does. A few rows beyond the grid row updated early is harmless.
    const size_t head_rows = in.has_prev ? round_up((size_t)in.halo) : 0;
    const size_t tail_start = in.has_next ? round_down(nl - (size_t)in.halo) : nl;
    // the pipeline needs the direction ring (its one-launch direction update writes out of place) and a slab thick enough to
    // have rows between its edge ranges; the in-place form and thinner slabs take the plain order
    L.pipeline = L.multi && !L.detail && !in.no_overlap && L.slots > 1 && in.reduce_scratch && (nl % 2) == 0 &&
                 nl >= 4 * (size_t)in.halo + 4 * kUnit && head_rows < tail_start;
    if (L.pipeline) L.head_rows = head_rows, L.tail_start = tail_start;
    L.bulk_lo = L.pipeline ? head_rows : 0, L.bulk_hi = L.pipeline ? tail_start : nl;
    return L;
}

// Iteration 0 of a solve of `max_iters` iterations under LoopShape::first_recomputed: where r0 lies decides the r update's instance.
// Stored: A p0 is stored and read back, the launches of before (first_recomputed off; a solve of no iterations launches none of this
// and keeps the launch that only sums r0.r0). FromB: b is r0 and p0 (b_is_p0), the first launch on b stores nothing on its fast
// blocks and the out-of-place instance reads b. FromSlot0: r0 lies in ring slot 0 alone (r0_in_ring), the block kernel stores nothing
// there and the out-of-place instance reads the slot. InPlace: r0 lies in r AND in slot 0 (stored twice), the in-loop instance on
// (r, p = slot 0) does it.
enum class FirstForm { Stored, FromB, FromSlot0, InPlace };
inline FirstForm first_form(const LoopShape& L, int max_iters) {
    if (!L.first_recomputed || max_iters <= 0) return FirstForm::Stored;
    return L.b_is_p0 ? FirstForm::FromB : L.r0_in_ring ? FirstForm::FromSlot0 : FirstForm::InPlace;
}

// what a flush of x starts from in the solve's first window: nothing (0.0 in registers) where x0 holds the library's own zeros
inline bool flush_skips_x0(bool x0_known_zero, int zero_start_parts) { return x0_known_zero && (zero_start_parts & 4) != 0; }

// ---- one iteration's small decisions (`enqueued`: iterations stepped so far, the one just stepped included) ----
// the sweep direction of iteration `index` (0-based): it flips every iteration; iteration 0 follows the forward initial pass
inline bool sweeps_backward(int index) { return (index & 1) == 0; }
// The scalar step rides in the direction update's launch (pipeline, all-reduce as a call of its own) -- except in the iteration
// whose new direction re-uses a slot the pending x flush still has to read: the flush needs this step's alpha first.
inline bool step_in_direction(bool pipeline, bool separate, int enqueued_before_step, int window_start, int slots) {
    return pipeline && separate && (enqueued_before_step + 1) - window_start < slots;
}
// the slot the new direction goes to still holds p of iteration enqueued - slots: the whole window is folded into x first
inline bool flush_due(int enqueued, int window_start, int slots) { return enqueued - window_start == slots; }

// ---- run-ahead and verdicts ----
// The LAB build's hooks; the product passes LabHooks{}. stop_at = k: iteration k counts as the converging one whatever its
// residual. guess_far_always: every iteration is guessed "cannot converge".
struct LabHooks { int stop_at = 0; bool guess_far_always = false; };
// What the host knows of a solve: the residual history in host-coherent memory (hist[0] = ||b||, hist[k] = ||r_k||, written before
// record k is published), its capacity, the tolerance.
struct StatusView { const double* hist; int hist_cap; double tolerance; LabHooks lab; };

// Is iteration `iteration` (1-based) too far from the tolerance to be the converging one? Judged by the residual of iteration
// `basis`, which the host has SEEN (basis <= records_read): CG on these systems halves the residual per iteration; a drop of 16 x
// per iteration between the known residual and `iteration` is the margin. A wrong guess costs empty dispatches, never a result:
// every kernel tests the flag itself.
inline bool far_from_convergence(const StatusView& v, int records_read, int iteration, int basis) {
    if (v.lab.guess_far_always) return true;
    if (v.lab.stop_at > 0) return iteration + 3 < v.lab.stop_at;  // behave like a solve that converges there
    if (basis < 0 || basis > records_read || basis >= v.hist_cap || iteration <= basis) return false;
    const double ratio = basis == 0 ? 1.0 : v.hist[basis] / v.hist[0];  // ||r0|| itself may not have been written yet
    double bar = v.tolerance;
    for (int k = basis; k < iteration; ++k) bar *= 16.0;
    return ratio > bar;  // (a NaN compares false: "may converge", the careful path)
}

// The verdict on iteration k (1-based, k <= records_read) from the history: the GPU's own test (sqrt(rr_new) / b_norm < tol,
// strict) on the same two doubles. Outside the history the last record's flag stands.
inline bool converged_at(const StatusView& v, bool record_flag, int k) {
    if (k < 1 || k >= v.hist_cap) return record_flag;
    if (v.lab.stop_at > 0 && k == v.lab.stop_at) return true;
    return v.hist[k] / v.hist[0] < v.tolerance;
}

// read_status for iteration j (1-based, just enqueued), in this order:
// 1. a host that ran ahead first catches up on record j - 1 ...
inline bool catches_up(int records_read, int j) { return records_read < j - 1; }
// 2. ... and if that iteration converged, the guess was wrong: iteration j was enqueued for nothing and the loop ends
inline bool ends_after_catch_up(const StatusView& v, bool record_flag, int j) { return converged_at(v, record_flag, j - 1); }
// 3. record j is awaited, or deferred: the host goes on to enqueue iteration j + 1 and reads the record on the way. Basis j - 1
// is the one residual every rank is sure to have (the decision must be the same on every rank); verbose >= 2 prints every
// iteration's scalars, and the last slot of the history is never run past.
inline bool defers_record(const StatusView& v, bool run_ahead, int verbose, int records_read, int j) {
    return run_ahead && verbose < 2 && j + 1 < v.hist_cap && far_from_convergence(v, records_read, j, j - 1);
}

// ---- the direction update's pieces (late bulk) ----
// lead piece + status record + rest: only on a range of at least four lead pieces, and only in iterations that MAY converge.
inline bool two_pieces(bool late, size_t lo, size_t hi, size_t lead_rows, bool predicted_far) {
    return late && hi - lo >= 4 * lead_rows && !predicted_far;
}
// first piece: the rows the sweep walks first -- [cut, hi) walking backward, [lo, cut) walking forward; the rest is the other side
// of the cut. One piece: `first` is all of [lo, hi).
struct Pieces { size_t first_lo, first_rows, rest_lo, rest_rows; };
inline Pieces direction_pieces(size_t lo, size_t hi, size_t lead_rows, bool backward, bool two) {
    const size_t cut = !two ? (backward ? lo : hi) : backward ? round_down(hi - lead_rows) : lo + lead_rows;
    return backward ? Pieces{cut, hi - cut, lo, cut - lo} : Pieces{lo, cut - lo, cut, hi - cut};
}

}  // namespace slab
}  // namespace spmv_amd
#endif
