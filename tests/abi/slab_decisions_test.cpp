// Stand-alone CPU test of csrc/slab_decisions.hpp: the CG slab solver's decisions -- the loop's shape, the run-ahead rules, the cut
// of the direction update, creation's arithmetic -- against values written out from the rules or an independent
// brute-force statement, never taken from the function under test. tests/test_host_logic.py builds it under
// -fsanitize=address,undefined and runs it; it prints "slab_decisions: ok" and returns 0, or names every check that failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "slab_decisions.hpp"

using namespace spmv_amd::slab;

static int failures = 0;
template <class... Args>
static void report(int line, const char* what, const char* format = "", Args... args) {
    ++failures;
    std::fprintf(stderr, "%s:%d: %s  [", __FILE__, line, what);
    if constexpr (sizeof...(Args) > 0) std::fprintf(stderr, format, args...);
    std::fprintf(stderr, "]\n");
}
#define CHECK(cond) ((cond) ? (void)0 : report(__LINE__, #cond))
#define CHECK_AT(cond, ...) ((cond) ? (void)0 : report(__LINE__, #cond, __VA_ARGS__))

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

// ---------------------------------------------------------------- run-ahead: the two predicates
static void test_far_and_verdict() {
    const double tol = 1e-6;
    std::vector<double> h = {2.0, 1.0, 0.5, 0.25, 0.125, 1e-3, 1e-9, 1e-9};  // hist[0] = ||b||
    const int cap = (int)h.size();
    StatusView v{h.data(), cap, tol, LabHooks{}};
    // the plain case: 0.25 / 2 against 1e-6 * 16
    CHECK(far_from_convergence(v, /*records_read=*/3, /*iteration=*/4, /*basis=*/3));
    // "may converge" (false) on every doubt
    CHECK(!far_from_convergence(v, 3, 4, -1));   // basis < 0
    CHECK(!far_from_convergence(v, 2, 4, 3));    // basis > records_read
    CHECK(!far_from_convergence(v, 9, 9, cap));  // basis >= hist_cap
    CHECK(!far_from_convergence(v, 9, 12, cap + 2));
    CHECK(!far_from_convergence(v, 3, 3, 3));  // iteration <= basis
    CHECK(!far_from_convergence(v, 3, 2, 3));
    for (double bad : {kNaN, kInf, -kInf}) {  // an entry that is not finite: NaN compares false, x / Inf is 0, Inf / Inf is NaN
        std::vector<double> g = h;
        StatusView w{g.data(), cap, tol, LabHooks{}};
        g[0] = bad;
        CHECK_AT(!far_from_convergence(w, 3, 4, 3), "hist[0] %g", bad);
        g = h, g[3] = bad;
        if (bad != kInf) CHECK_AT(!far_from_convergence(w, 3, 4, 3), "hist[basis] %g", bad);
        g[0] = bad;
        CHECK_AT(!far_from_convergence(w, 3, 4, 3), "hist[0] and hist[basis] %g", bad);
    }
    {  // The one case in which a non-finite entry does NOT give the careful path, with today's answer (the rule was moved as it is):
        // +Inf as the known residual over a finite ||b|| is "far", so record 4 is deferred once. The residual after an Inf is NaN
        // (Inf - Inf in the next update), which is awaited, and every kernel tests the flag itself: no result depends on it.
        std::vector<double> g = h;
        g[3] = kInf;
        StatusView w{g.data(), cap, tol, LabHooks{}};
        CHECK(far_from_convergence(w, 3, 4, 3));
        g[4] = kNaN;
        CHECK(!far_from_convergence(w, 4, 5, 4));
    }
    {  // basis 0 does not read hist[0] (||r0|| may not have been written yet): the ratio is 1
        std::vector<double> g = {kNaN, kNaN, kNaN};
        StatusView w{g.data(), 3, tol, LabHooks{}};
        CHECK(far_from_convergence(w, 0, 1, 0));
        StatusView loose{g.data(), 3, 0.07, LabHooks{}};  // 1 > 0.07 * 16 is false
        CHECK(!far_from_convergence(loose, 0, 1, 0));
    }
    {  // tolerance 0: the bar is 0, every positive known residual defers; a residual of exactly 0 does not
        StatusView w{h.data(), cap, 0.0, LabHooks{}};
        for (int b = 0; b + 1 < cap; ++b) CHECK_AT(far_from_convergence(w, b, b + 1, b), "basis %d", b);
        std::vector<double> g = {2.0, 0.0, 0.0};
        StatusView z{g.data(), 3, 0.0, LabHooks{}};
        CHECK(!far_from_convergence(z, 1, 2, 1));
    }
    {  // the 16 x margin: bar = tol * 16^(iteration - basis), strict >. Powers of two keep every product exact.
        const double t = std::ldexp(1.0, -20);
        for (int steps = 1; steps <= 3; ++steps) {
            const double bar = std::ldexp(t, 4 * steps);
            std::vector<double> g = {1.0, bar, 0.0, 0.0, 0.0};
            StatusView w{g.data(), 5, t, LabHooks{}};
            CHECK_AT(!far_from_convergence(w, 1, 1 + steps, 1), "at the bar, %d steps", steps);
            g[1] = std::nextafter(bar, 2.0);
            CHECK_AT(far_from_convergence(w, 1, 1 + steps, 1), "just above the bar, %d steps", steps);
            g[1] = std::nextafter(bar, 0.0);
            CHECK_AT(!far_from_convergence(w, 1, 1 + steps, 1), "just below the bar, %d steps", steps);
        }
    }
    // converged_at: the record's flag outside [1, hist_cap), strict < inside
    for (bool flag : {false, true}) {
        CHECK(converged_at(v, flag, 0) == flag);
        CHECK(converged_at(v, flag, -3) == flag);
        CHECK(converged_at(v, flag, cap) == flag);
        CHECK(converged_at(v, flag, cap + 5) == flag);
        CHECK(!converged_at(v, flag, 5));  // 1e-3 / 2
        CHECK(converged_at(v, flag, 6));   // 1e-9 / 2
    }
    {
        const double t = std::ldexp(1.0, -20);
        std::vector<double> g = {4.0, 4.0 * t, std::nextafter(4.0 * t, 0.0), kNaN};
        StatusView w{g.data(), 4, t, LabHooks{}};
        CHECK(!converged_at(w, true, 1));  // equal is not below
        CHECK(converged_at(w, false, 2));
        CHECK(!converged_at(w, true, 3));  // NaN never converges
    }
    // the LAB build's hooks, as today's code: guess_far_always wins; stop_at = k replaces the residual rule by "iteration + 3 < k"
    {
        StatusView w{h.data(), cap, tol, LabHooks{0, true}};
        CHECK(far_from_convergence(w, 0, 1, -1) && far_from_convergence(w, 6, 7, 6));
        StatusView st{h.data(), cap, tol, LabHooks{14, false}};
        CHECK(far_from_convergence(st, 3, 10, 3) && !far_from_convergence(st, 3, 11, 3) && !far_from_convergence(st, 3, 14, 3));
        CHECK(far_from_convergence(st, 0, 10, 99));  // the basis is not looked at
        StatusView s4{h.data(), cap, tol, LabHooks{4, false}};
        CHECK(converged_at(s4, false, 4) && !converged_at(s4, false, 3));
        CHECK(converged_at(s4, false, 6));  // the residual rule still holds elsewhere
        StatusView s9{h.data(), cap, tol, LabHooks{cap, false}};
        CHECK(!converged_at(s9, false, cap) && converged_at(s9, true, cap));  // outside the history the flag stands, stop_at or not
    }
    // defers_record: never with verbose >= 2, never on the history's last slot, never with run-ahead off
    CHECK(defers_record(v, true, 0, 3, 4) && defers_record(v, true, 1, 3, 4));
    CHECK(!defers_record(v, true, 2, 3, 4) && !defers_record(v, true, 3, 3, 4));
    CHECK(!defers_record(v, false, 0, 3, 4));
    {
        StatusView w{h.data(), 5, tol, LabHooks{}};  // j + 1 == hist_cap
        CHECK(!defers_record(w, true, 0, 3, 4));
        StatusView w6{h.data(), 6, tol, LabHooks{}};
        CHECK(defers_record(w6, true, 0, 3, 4));
    }
    CHECK(!defers_record(v, true, 0, 2, 4));  // record j - 1 not read: no basis
    CHECK(catches_up(0, 2) && !catches_up(1, 2) && !catches_up(0, 1) && !catches_up(5, 3));
    CHECK(ends_after_catch_up(v, false, 7) && !ends_after_catch_up(v, true, 6));  // the verdict on j - 1, from the history
}

// ---------------------------------------------------------------- the loop as a whole, simulated
// The GPU's side of a solve: it works through the iterations the host enqueued, in order; an iteration behind the converging one
// only publishes its record. `lazy`: it works exactly as far as the host waits (an entry of the history the host did not wait
// for still holds what the previous solve, or nobody, left there); otherwise everything enqueued has run.
struct SimSlab {  // what outlives a solve on one slab
    std::vector<double> hist;
    int poll_sequence = 0;
    int published = 0, flag = 0, iterations = 0;
};
struct SimGpu {
    SimSlab& s;
    const std::vector<double>& truth;  // truth[0] = ||b||, truth[k] = ||r_k||
    double tol;
    int sequence0, done = 0;
    void run_to(int k) {
        for (; done < k; ++done) {
            const int i = done + 1;
            s.published = sequence0 + i;
            if (s.flag) continue;
            s.hist[0] = truth[0];
            if (i < (int)s.hist.size()) s.hist[i] = truth[i];
            s.iterations = i;
            s.flag = truth[i] / truth[0] < tol ? 1 : 0;
        }
    }
};
struct Outcome {
    int iterations, converged, enqueued;
};
// the converging iteration by definition, and a host that awaits every record
static Outcome careful(const std::vector<double>& truth, double tol, int max_iters) {
    for (int k = 1; k <= max_iters; ++k)
        if (truth[k] / truth[0] < tol) return Outcome{k, 1, k};
    return Outcome{max_iters, 0, max_iters};
}
// spmv_amd_cg_slab_solve's loop with SolveRun::read_status's decisions (late bulk off)
static Outcome run_ahead(SimSlab& s, const std::vector<double>& truth, double tol, int max_iters, bool lazy, int verbose) {
    SimGpu gpu{s, truth, tol, s.poll_sequence};
    s.flag = 0, s.iterations = 0;
    const StatusView view{s.hist.data(), (int)s.hist.size(), tol, LabHooks{}};
    int records_read = 0, enqueued = 0;
    const auto await = [&](int k) {
        gpu.run_to(k);
        CHECK_AT(s.published - (gpu.sequence0 + k) >= 0, "record %d was never enqueued", k);
        if (k > records_read) records_read = k;
    };
    bool done = false;
    while (!done && enqueued < max_iters) {
        ++s.poll_sequence, ++enqueued;
        if (!lazy) gpu.run_to(enqueued);
        const int j = enqueued;
        if (catches_up(records_read, j)) {
            await(j - 1);
            if (ends_after_catch_up(view, s.flag != 0, j)) {
                await(j);
                break;
            }
        }
        const bool deferred = defers_record(view, true, verbose, records_read, j);
        if (!deferred) await(j);
        done = deferred ? false : s.flag != 0;
    }
    gpu.run_to(enqueued);  // finish() drains the stream
    return Outcome{s.iterations, s.flag, enqueued};
}

static void check_history(const char* name, const std::vector<double>& truth, double tol, int max_iters) {
    const Outcome want = careful(truth, tol, max_iters);
    for (int extra_cap : {0, 7})  // a history that an earlier, longer solve left larger than max_iters + 1
        for (bool lazy : {true, false})
            for (int verbose : {0, 2}) {
                SimSlab s;
                s.hist.assign((size_t)(want_hist(max_iters) + extra_cap), 0.0);  // zeros: an entry read too early looks converged
                s.poll_sequence = 40;
                for (int solve = 0; solve < 3; ++solve) {  // the same system again on the same slab, poll_sequence carried over
                    const Outcome got = run_ahead(s, truth, tol, max_iters, lazy, verbose);
                    CHECK_AT(got.iterations == want.iterations && got.converged == want.converged, "%s cap+%d lazy %d verbose %d solve %d: %d/%d, want %d/%d",
                             name, extra_cap, lazy, verbose, solve, got.iterations, got.converged, want.iterations, want.converged);
                    CHECK_AT(got.enqueued >= want.enqueued, "%s: ended at %d before %d", name, got.enqueued, want.enqueued);
                    CHECK_AT(got.enqueued <= want.enqueued + 1 && got.enqueued <= max_iters, "%s: enqueued %d for %d", name, got.enqueued, want.enqueued);
                    if (verbose >= 2) CHECK_AT(got.enqueued == want.enqueued, "%s: verbose 2 ran ahead", name);
                }
            }
}

static void test_simulated_loops() {
    const double tol = 1e-6;
    const auto halving = [](int n) {
        std::vector<double> t((size_t)n + 1);
        for (int k = 0; k <= n; ++k) t[(size_t)k] = 3.0 * std::ldexp(1.0, -k);
        return t;
    };
    check_history("steady halving", halving(40), tol, 40);  // 2^-20 < 1e-6: iteration 20
    CHECK(careful(halving(40), tol, 40).iterations == 20);
    for (int d = 1; d <= 20; ++d) {  // a drop of 100 x in one step, at each iteration up to where halving alone converges
        std::vector<double> t = halving(40);
        for (int k = d; k <= 40; ++k) t[(size_t)k] *= 0.01;
        check_history("drop of 100x", t, tol, 40);
    }
    {
        std::vector<double> t = halving(10);
        t[1] = 1e-9;
        check_history("converges at iteration 1", t, tol, 10);
        check_history("converges at iteration 1, max_iters 1", t, tol, 1);
    }
    {
        std::vector<double> t(31);
        for (int k = 0; k <= 30; ++k) t[(size_t)k] = std::pow(0.999, k);
        check_history("no convergence before max_iters", t, tol, 30);  // every record deferred, the last iteration included (cap + 7)
    }
    for (int cut = 1; cut <= 21; ++cut) check_history("max_iters cuts the solve", halving(40), tol, cut);
    for (int k = 1; k <= 12; ++k) {  // NaN from iteration k on: never converges, and is never run ahead of
        std::vector<double> t = halving(12);
        for (int i = k; i <= 12; ++i) t[(size_t)i] = kNaN;
        check_history("NaN appears", t, tol, 12);
    }
    check_history("tolerance 0", halving(25), 0.0, 25);
}

// ---------------------------------------------------------------- the loop's shape
static ShapeInputs slab_with_neighbours(size_t n_local, int halo) {  // takes the pipeline
    ShapeInputs in{};
    in.exchanges_halos = in.collective = true, in.mailbox_ready = false;
    in.ring_slots = 16, in.n_local = n_local, in.halo = halo, in.has_prev = in.has_next = true;
    in.owns_matrix = true, in.reduce_scratch = true;
    in.fused_direction = 1, in.fused_dot = true, in.fuse_init_residual = true, in.zero_start_parts = 7;
    return in;
}
static ShapeInputs slab_alone() {  // takes the direction update inside the block SpMV and both ends of zero_start
    ShapeInputs in = slab_with_neighbours(1 << 20, 0);
    in.exchanges_halos = in.collective = in.has_prev = in.has_next = false;
    in.planes_and_classes = in.block_plan = true, in.slow_blocks = 4, in.block_tiles = 64;
    in.late_bulk = true, in.x0_known_zero = true;
    return in;
}

static void test_shape() {
    const ShapeInputs ok = slab_with_neighbours(1 << 20, 1000);
    {
        const LoopShape L = loop_shape(ok);
        CHECK(L.pipeline && L.multi && L.reduce && L.separate && !L.use_mailbox && !L.detail && L.slots == 16);
        CHECK(L.head_rows == 1024 && L.tail_start == ((1u << 20) - 1000) / 512 * 512 && L.bulk_lo == 1024 && L.bulk_hi == L.tail_start);
        ShapeInputs in = ok;
        in.mailbox_ready = true;
        CHECK(loop_shape(in).use_mailbox && !loop_shape(in).separate && loop_shape(in).pipeline);
        in.collective = false;
        CHECK(!loop_shape(in).use_mailbox && !loop_shape(in).separate && !loop_shape(in).reduce);
    }
    const auto refused = [&](const char* why, ShapeInputs in) {
        const LoopShape L = loop_shape(in);
        CHECK_AT(!L.pipeline && L.bulk_lo == 0 && L.bulk_hi == in.n_local && L.head_rows == 0 && L.tail_start == 0, "%s", why);
    };
    ShapeInputs in = ok;
    in.n_local += 1, refused("odd n_local", in), in = ok;
    in.ring_slots = 1, refused("ring 1", in), in = ok;
    in.detailed_timers = true, refused("detailed timers", in), in = ok;
    in.no_overlap = true, refused("no_overlap", in), in = ok;
    in.reduce_scratch = false, refused("no reduction scratch", in), in = ok;
    in.exchanges_halos = false, refused("no halos to exchange", in), in = ok;
    for (int halo : {1, 511, 512, 513, 14142, 20000}) {  // thick enough from 4 * halo + 2048 rows on
        const size_t edge = 4 * (size_t)halo + 2048;
        CHECK_AT(loop_shape(slab_with_neighbours(edge, halo)).pipeline, "halo %d at the boundary", halo);
        refused("two rows thinner than the boundary", slab_with_neighbours(edge - 2, halo));
    }
    for (int halo : {1, 511, 512, 513, 14142, 20000})
        for (size_t n_local : {4 * (size_t)halo + 2048, 4 * (size_t)halo + 2050, 4 * (size_t)halo + 3072, 10 * (size_t)halo + 5000, (size_t)100000000})
            for (int sides = 0; sides < 4; ++sides) {
                ShapeInputs s = slab_with_neighbours(n_local, halo);
                s.has_prev = (sides & 1) != 0, s.has_next = (sides & 2) != 0;
                const LoopShape L = loop_shape(s);
                CHECK_AT(L.pipeline, "halo %d n_local %zu sides %d", halo, n_local, sides);
                // [0, head_rows) | bulk | [tail_start, n_local) partition the slab
                CHECK_AT(L.bulk_lo == L.head_rows && L.bulk_hi == L.tail_start && L.head_rows <= L.tail_start && L.tail_start <= n_local,
                         "halo %d n_local %zu sides %d: %zu %zu", halo, n_local, sides, L.head_rows, L.tail_start);
                if (s.has_prev) CHECK_AT(L.head_rows % 512 == 0 && L.head_rows >= (size_t)halo && L.head_rows < (size_t)halo + 512, "head %zu halo %d", L.head_rows, halo);
                else CHECK(L.head_rows == 0);
                if (s.has_next) CHECK_AT(L.tail_start % 512 == 0 && n_local - L.tail_start >= (size_t)halo && n_local - L.tail_start < (size_t)halo + 512,
                                         "tail %zu halo %d n_local %zu", L.tail_start, halo, n_local);
                else CHECK(L.tail_start == n_local);
            }
    // the direction update inside the block SpMV
    const ShapeInputs alone = slab_alone();
    {
        const LoopShape L = loop_shape(alone);
        CHECK(L.fused_direction && !L.late && L.zero_start && L.r0_in_ring && !L.pipeline && !L.multi && L.bulk_lo == 0 && L.bulk_hi == alone.n_local);
    }
    const auto fused = [](ShapeInputs s) { return loop_shape(s).fused_direction; };
    in = alone, in.exchanges_halos = true, CHECK(!fused(in));
    in = alone, in.owns_matrix = false, CHECK(!fused(in));
    in = alone, in.ring_slots = 1, CHECK(!fused(in));
    in = alone, in.detailed_timers = true, CHECK(!fused(in));
    in = alone, in.fused_direction = 0, CHECK(!fused(in));
    in = alone, in.fused_dot = false, CHECK(!fused(in));
    in = alone, in.planes_and_classes = false, CHECK(!fused(in));
    in = alone, in.block_plan = false, CHECK(!fused(in));
    in = alone, in.slow_blocks = 4, in.block_tiles = 64, CHECK(fused(in));  // 16 * slow == tiles
    in.slow_blocks = 5, CHECK(!fused(in));
    in.fused_direction = 2, CHECK(fused(in));  // option 2 ignores the cap
    in.slow_blocks = -1, CHECK(!fused(in));    // the slow blocks could not be listed
    in.fused_direction = 1, CHECK(!fused(in));
    in = alone, in.slow_blocks = 0, in.block_tiles = 0, CHECK(fused(in));
    CHECK(direction_spmv_available(alone, true) && direction_spmv_available(alone, false));
    in = alone, in.slow_blocks = 60, CHECK(!direction_spmv_available(in, true) && direction_spmv_available(in, false));
    // late bulk: only without the fused direction update, with the ring, without detailed timers
    in = alone, in.fused_direction = 0, CHECK(loop_shape(in).late);
    in.late_bulk = false, CHECK(!loop_shape(in).late);
    in = alone, in.fused_direction = 0, in.ring_slots = 1, CHECK(!loop_shape(in).late);
    in = alone, in.fused_direction = 0, in.detailed_timers = true, CHECK(!loop_shape(in).late);
    for (int option = 0; option <= 2; ++option)
        for (int slow : {-1, 0, 4, 5, 64}) {
            in = alone, in.fused_direction = option, in.slow_blocks = slow;
            const LoopShape L = loop_shape(in);
            CHECK_AT(!(L.late && L.fused_direction) && (L.late || L.fused_direction), "option %d slow %d", option, slow);
        }
    // the two ends of a solve
    const auto ends = [](ShapeInputs s) { const LoopShape L = loop_shape(s); return (L.zero_start ? 1 : 0) | (L.r0_in_ring ? 2 : 0); };
    CHECK(ends(alone) == 3);
    in = alone, in.x0_known_zero = false, CHECK(ends(in) == 2);
    in = alone, in.zero_start_parts = 6, CHECK(ends(in) == 2);
    in = alone, in.zero_start_parts = 5, CHECK(ends(in) == 1);
    in = alone, in.zero_start_parts = 4, CHECK(ends(in) == 0);
    in = alone, in.zero_start_parts = 0, CHECK(ends(in) == 0);
    in = alone, in.x0_known_zero = false, in.zero_start_parts = 2, CHECK(ends(in) == 2);  // r0_in_ring needs only its bit
    in = alone, in.exchanges_halos = true, CHECK(ends(in) == 0);
    in = alone, in.ring_slots = 1, CHECK(ends(in) == 0);
    in = alone, in.fuse_init_residual = false, CHECK(ends(in) == 0);
    in = alone, in.owns_matrix = false, CHECK(ends(in) == 0);
    CHECK(flush_skips_x0(true, 7) && flush_skips_x0(true, 4) && !flush_skips_x0(true, 3) && !flush_skips_x0(false, 7) && !flush_skips_x0(true, 0));
}

// ---------------------------------------------------------------- the direction update's pieces and the iteration's one-liners
static void test_pieces() {
    for (size_t lo : {(size_t)0, (size_t)512, (size_t)20480})
        for (size_t lead : {(size_t)512, (size_t)1024, (size_t)1 << 15})
            for (size_t len : {(size_t)0, (size_t)2, 4 * lead - 2, 4 * lead, 4 * lead + 2, 4 * lead + 777 * 2, 64 * lead + 510})
                for (bool backward : {false, true})
                    for (bool late : {false, true})
                        for (bool far : {false, true}) {
                            const size_t hi = lo + len;
                            const bool two = two_pieces(late, lo, hi, lead, far);
                            CHECK_AT(two == (late && !far && len >= 4 * lead), "lo %zu len %zu lead %zu", lo, len, lead);
                            const Pieces p = direction_pieces(lo, hi, lead, backward, two);
                            // first + rest partition [lo, hi); the first piece is where the sweep starts
                            const size_t a = backward ? p.rest_lo : p.first_lo, a_rows = backward ? p.rest_rows : p.first_rows;
                            const size_t b = backward ? p.first_lo : p.rest_lo, b_rows = backward ? p.first_rows : p.rest_rows;
                            CHECK_AT(a == lo && a + a_rows == b && b + b_rows == hi, "lo %zu len %zu lead %zu backward %d two %d", lo, len, lead, backward, two);
                            if (!two) CHECK_AT(p.first_rows == len && p.rest_rows == 0, "one piece: lo %zu len %zu lead %zu backward %d", lo, len, lead, backward);
                            else if (backward) CHECK_AT(p.first_lo % 512 == 0 && p.first_rows >= lead && p.first_rows < lead + 512 && p.rest_rows > 0, "backward cut %zu", p.first_lo);
                            else CHECK_AT(p.first_rows == lead && p.rest_rows == len - lead, "forward cut %zu", p.rest_lo);
                        }
    // step_in_direction: the step rides in the direction launch unless the new direction re-uses a slot the pending flush reads
    for (int slots : {2, 3, 16})
        for (int window_start : {0, slots, 5 * slots})
            for (int k = 0; k < slots; ++k) {  // k iterations of the window stepped before this one
                const int enqueued = window_start + k;
                CHECK_AT(step_in_direction(true, true, enqueued, window_start, slots) == (k + 1 < slots), "slots %d window %d k %d", slots, window_start, k);
                CHECK(!step_in_direction(false, true, enqueued, window_start, slots) && !step_in_direction(true, false, enqueued, window_start, slots));
                // ... and that iteration is the one whose direction stage flushes the window first
                CHECK_AT(flush_due(enqueued + 1, window_start, slots) == (k + 1 == slots), "slots %d window %d k %d", slots, window_start, k);
            }
    CHECK(sweeps_backward(0) && !sweeps_backward(1) && sweeps_backward(2));
    // want_hist: one slot per iteration and one for ||r0||, capped at 2^20
    CHECK(want_hist(0) == 1 && want_hist(14) == 15 && want_hist((1 << 20) - 2) == (1 << 20) - 1);
    CHECK(want_hist((1 << 20) - 1) == (1 << 20) && want_hist(1 << 20) == (1 << 20) && want_hist(2000000000) == (1 << 20));
}

// ---------------------------------------------------------------- creation's arithmetic
static void test_creation() {
    const size_t k2MiB = (size_t)2 << 20, GiB = (size_t)1 << 30;
    CHECK(round_up(0) == 0 && round_up(1) == 512 && round_up(512) == 512 && round_up(513) == 1024);
    CHECK(round_down(0) == 0 && round_down(511) == 0 && round_down(512) == 512 && round_down(1023) == 512);
    for (int halo : {0, 1, 511, 512, 513, 14142, 20000})
        for (size_t n_local : {(size_t)2, (size_t)4096, (size_t)262143, (size_t)262144, (size_t)200000000, (size_t)400000000}) {
            const SlotLayout l = slot_layout(n_local, halo);
            CHECK_AT(l.lead % 512 == 0 && l.lead >= (size_t)halo && l.lead < (size_t)halo + 512, "lead %zu halo %d", l.lead, halo);
            CHECK_AT(l.slot_doubles == l.lead + n_local + (size_t)halo + 2, "slot %zu", l.slot_doubles);
            const size_t bytes = l.pitch * sizeof(double);
            CHECK_AT(bytes % k2MiB == 4096 && l.pitch >= l.slot_doubles && bytes < l.slot_doubles * sizeof(double) + k2MiB + 4096, "pitch %zu for slot %zu", l.pitch, l.slot_doubles);
        }
    {
        const PlaneLayout p = plane_layout(1000, 100);  // [C, E]: 2000 -> 2048; the S plane's halo row: 100 -> 512
        CHECK(p.ce == 2048 && p.halo_lead == 512 && p.s_offset == 2560 && p.total == 3560);
        const PlaneLayout q = plane_layout((size_t)400000000, 20000);
        CHECK(q.ce == 800000000 && q.halo_lead == 20480 && q.s_offset == 800020480 && q.total == 1200020480);
    }
    {  // the planes: beside r, Ap, the first buffer and a ring of 4, with 4 GiB left; strict >
        const size_t per = 3 * GiB + 4096, planes = 9 * GiB;
        const size_t needed = planes + 4 * GiB + 6 * per;
        CHECK(planes_fit(needed + 1, planes, per) && !planes_fit(needed, planes, per) && !planes_fit(0, planes, per));
    }
    CHECK(may_take_planes(true, 640, 512, 640 * 10, 640 * 3));
    CHECK(!may_take_planes(false, 640, 512, 6400, 0) && !may_take_planes(true, 300, 512, 3000, 0) && !may_take_planes(true, 640, 512, 6401, 0));
    CHECK(!may_take_planes(true, 640, 512, 6400, 5) && !may_take_planes(true, 640, 512, 0, 0) && !may_take_planes(true, 1, 0, 4, 0) && !may_take_planes(true, -1, 0, 4, 0));
    CHECK(may_take_planes(true, 2, 0, 4, 0));
    {  // the ring. A slab that owns its matrix: what is free beyond 4 GiB and r, Ap, the first buffer
        const size_t per = GiB + 4096, base = 4 * GiB + 3 * per, plenty = (size_t)200 * GiB;
        CHECK(ring_length(0, per, plenty, false, 16) == 1 && ring_length(-7, per, plenty, false, 16) == 1 && ring_length(1, per, plenty, false, 16) == 1);
        CHECK(ring_length(16, per, plenty, false, 16) == 16 && ring_length(17, per, plenty, false, 16) == 16 && ring_length(5, per, plenty, false, 16) == 5);
        CHECK(ring_length(16, per, base + 15 * per, false, 16) == 16);
        CHECK(ring_length(16, per, base + 15 * per - 1, false, 16) == 15);  // 15 fit: a ring of 15
        CHECK(ring_length(16, per, base + 3 * per, false, 16) == 4);
        CHECK(ring_length(16, per, base + 3 * per - 1, false, 16) == 1);  // 3 fit: cut short below 4, the in-place form
        CHECK(ring_length(16, per, base, false, 16) == 1 && ring_length(16, per, base - 1, false, 16) == 1 && ring_length(16, per, 0, false, 16) == 1);
        CHECK(ring_length(3, per, base + 2 * per, false, 16) == 3);      // asked for 3 and got 3: not cut short
        CHECK(ring_length(3, per, base + 2 * per - 1, false, 16) == 1);  // asked for 3, 2 fit
        CHECK(ring_length(2, per, base + per - 1, false, 16) == 1 && ring_length(2, per, base + per, false, 16) == 2);
        // a borrowed operator: a quarter of what is free, nothing set aside
        CHECK(ring_length(16, per, 4 * 15 * per, true, 16) == 16 && ring_length(16, per, 4 * 15 * per - 1, true, 16) == 15);
        CHECK(ring_length(16, per, 4 * 3 * per, true, 16) == 4 && ring_length(16, per, 4 * 3 * per - 1, true, 16) == 1);
        CHECK(ring_length(16, per, base + 15 * per, true, 16) == 6);  // what gives a slab of its own 16: (4 GiB + 18 per) / 4 = 5 per and a bit
        CHECK(ring_length(17, per, plenty, true, 16) == 16 && ring_length(0, per, plenty, true, 16) == 1);
    }
    // which sides have a neighbour: first, middle, last rank; one rank; the whole-grid self-neighbour probe; a stand-in slab
    const auto sides = [](bool halos, int rank, int world, bool self) { const Sides s = slab_sides(halos, rank, world, self, 777); return (s.has_prev ? 1 : 0) | (s.has_next ? 2 : 0) | (s.halo == 777 ? 4 : 0) | (s.halo == 0 ? 8 : 0); };
    CHECK(sides(true, 0, 4, false) == (2 | 4) && sides(true, 1, 4, false) == (1 | 2 | 4) && sides(true, 2, 4, false) == (1 | 2 | 4) && sides(true, 3, 4, false) == (1 | 4));
    CHECK(sides(false, 0, 1, false) == 8 && sides(false, 1, 4, false) == 8 && sides(false, 0, 1, true) == 8);
    CHECK(sides(true, 0, 1, true) == (1 | 2 | 4));   // the whole grid on a self-neighbour rank: halos on both sides
    CHECK(sides(true, 0, 1, false) == 4);            // ... and without the self-neighbour: none
    CHECK(sides(true, 0, 8, true) == (2 | 4) && sides(true, 7, 8, true) == (1 | 4) && sides(true, 3, 8, true) == (1 | 2 | 4));  // stand-in slabs keep their job's sides
    // the rows that need no halo
    const auto range = [](int n, int halo, bool prev, bool next) { const RowRange r = halo_free_rows(n, halo, prev, next); return r.lo * 100000 + r.hi; };
    CHECK(range(5000, 100, false, false) == 5000 && range(5000, 100, true, false) == 100 * 100000 + 5000);
    CHECK(range(5000, 100, false, true) == 4900 && range(5000, 100, true, true) == 100 * 100000 + 4900 && range(100, 100, true, true) == 100 * 100000);
    // the boundary rows ride in the reducing launch: in-loop form only, whole grid rows, at most one per side
    CHECK(fused_tail(true, true, false, 100, 100, 100) && fused_tail(true, true, false, 0, 100, 100) && fused_tail(true, true, false, 100, 0, 100));
    CHECK(!fused_tail(false, true, false, 100, 100, 100) && !fused_tail(true, false, false, 100, 100, 100) && !fused_tail(true, true, true, 100, 100, 100));
    CHECK(!fused_tail(true, true, false, 200, 100, 100) && !fused_tail(true, true, false, 100, 200, 100) && !fused_tail(true, true, false, 50, 100, 100) &&
          !fused_tail(true, true, false, 100, 99, 100));
    CHECK(partition_check(false, -1, 0) == Partition::Ok && partition_check(true, 0, 50) == Partition::NeedsStencil && partition_check(true, -1, 50) == Partition::NeedsStencil);
    CHECK(partition_check(true, 100, 99) == Partition::ThinnerThanGridRow && partition_check(true, 100, 100) == Partition::Ok);
    CHECK(!late_bulk_default(99999999) && late_bulk_default(100000000));
    CHECK(!wants_coefficient_placement(((size_t)16 << 20) - 1, 3) && wants_coefficient_placement((size_t)16 << 20, 2) && !wants_coefficient_placement((size_t)16 << 20, 1));
    CHECK(halo_wait_limit_s(2.0, 30.0) == 2.0 && halo_wait_limit_s(0.0, 30.0) == 15.0 && halo_wait_limit_s(0.0, 0.0) == 20.0 && halo_wait_limit_s(0.0, 40.0) == 20.0 &&
          halo_wait_limit_s(0.0, 39.0) == 19.5);
}

int main() {
    test_far_and_verdict();
    test_simulated_loops();
    test_shape();
    test_pieces();
    test_creation();
    if (failures) {
        std::fprintf(stderr, "slab_decisions: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("slab_decisions: ok\n");
    return 0;
}
