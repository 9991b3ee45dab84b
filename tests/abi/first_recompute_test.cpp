// Stand-alone CPU test of two decisions of csrc/slab_decisions.hpp: LoopShape::first_recomputed with first_form (iteration 0 leaves
// A p0 unstored and its r update recomputes it, from b, from ring slot 0 or in place) and default_block_rows (8-row block tiles where
// the fused loop can run, 4 elsewhere). Both truth tables are written out from the rules.
// tests/test_first_recompute_host.py builds it under -fsanitize=address,undefined and runs it; it prints "first_recompute: ok" and
// returns 0, or names every check that failed.
#include <cstdio>
#include <initializer_list>

#include "slab_decisions.hpp"

using namespace spmv_amd::slab;

static int failures = 0;
static void report(int line, const char* what) {
    ++failures;
    std::fprintf(stderr, "%s:%d: %s\n", __FILE__, line, what);
}
#define CHECK(cond) ((cond) ? (void)0 : report(__LINE__, #cond))

// a slab that takes every form the rule builds on: one rank, owns its matrix, ring of 4, the block kernel on the whole slab with an
// eligible block map, x0 = the library's zeros on a matrix whose rows sum to +0.0, every option at its default
static ShapeInputs eligible() {
    ShapeInputs in{};
    in.ring_slots = 4, in.n_local = 1 << 20, in.owns_matrix = true, in.reduce_scratch = true;
    in.fused_direction = 1, in.fused_dot = true, in.planes_and_classes = true, in.block_plan = true, in.slow_blocks = 4, in.block_tiles = 64;
    in.fuse_init_residual = true, in.x0_known_zero = true, in.zero_start_parts = 15, in.zero_rows_plus_zero = true;
    in.ap_recompute = 1, in.skew_eligible = true, in.first_recompute = 1;
    return in;
}
static FirstForm form(const ShapeInputs& in, int max_iters = 14) { return first_form(loop_shape(in), max_iters); }

static void test_first_recomputed() {
    const ShapeInputs ok = eligible();
    ShapeInputs in = ok;
    {
        const LoopShape L = loop_shape(ok);
        CHECK(L.fused_direction && L.ap_recomputed && L.first_recomputed && L.b_is_p0 && L.r0_in_ring && L.zero_start);
    }
    // where r0 lies picks the instance: b, ring slot 0, or r itself
    CHECK(form(ok) == FirstForm::FromB);
    in = ok, in.x0_known_zero = false, CHECK(form(in) == FirstForm::FromSlot0 && loop_shape(in).r0_in_ring && !loop_shape(in).b_is_p0);
    in = ok, in.zero_rows_plus_zero = false, CHECK(form(in) == FirstForm::FromSlot0);
    in = ok, in.zero_start_parts = 7, CHECK(form(in) == FirstForm::FromSlot0);  // b does not serve as p0
    in = ok, in.zero_start_parts = 5, CHECK(form(in) == FirstForm::InPlace && !loop_shape(in).r0_in_ring);  // r0 stored twice
    in = ok, in.zero_start_parts = 0, CHECK(form(in) == FirstForm::InPlace);
    in = ok, in.fuse_init_residual = false, CHECK(form(in) == FirstForm::InPlace);
    // the option, and everything ap_recomputed needs
    in = ok, in.first_recompute = 0, CHECK(form(in) == FirstForm::Stored && loop_shape(in).ap_recomputed && !loop_shape(in).first_recomputed);
    in = ok, in.ap_recompute = 0, CHECK(form(in) == FirstForm::Stored && !loop_shape(in).first_recomputed);
    in = ok, in.skew_eligible = false, CHECK(form(in) == FirstForm::Stored);
    in = ok, in.fused_direction = 0, CHECK(form(in) == FirstForm::Stored && loop_shape(in).b_is_p0);
    in = ok, in.slow_blocks = 64, CHECK(form(in) == FirstForm::Stored);  // more than 1 / 16 of the blocks are slow
    in = ok, in.slow_blocks = 64, in.fused_direction = 2, CHECK(form(in) == FirstForm::FromB);
    in = ok, in.detailed_timers = true, CHECK(form(in) == FirstForm::Stored);
    in = ok, in.ring_slots = 1, CHECK(form(in) == FirstForm::Stored);
    in = ok, in.owns_matrix = false, CHECK(form(in) == FirstForm::Stored);
    in = ok, in.exchanges_halos = true, CHECK(form(in) == FirstForm::Stored);
    in = ok, in.block_plan = false, CHECK(form(in) == FirstForm::Stored);
    // the whole table over (ap_recomputed, option, b_is_p0, r0_in_ring, max_iters == 0)
    for (int ap = 0; ap < 2; ++ap)
        for (int opt = 0; opt < 2; ++opt)
            for (int b = 0; b < 2; ++b)
                for (int ring = 0; ring < 2; ++ring)
                    for (int none = 0; none < 2; ++none) {
                        LoopShape L;
                        L.ap_recomputed = ap != 0, L.first_recomputed = ap != 0 && opt != 0, L.b_is_p0 = b != 0 && ring != 0, L.r0_in_ring = ring != 0;
                        const FirstForm want = !(ap && opt) || none ? FirstForm::Stored
                                               : L.b_is_p0          ? FirstForm::FromB
                                               : L.r0_in_ring       ? FirstForm::FromSlot0
                                                                    : FirstForm::InPlace;
                        CHECK(first_form(L, none ? 0 : 1) == want);
                        CHECK(first_form(L, none ? 0 : 14) == want);
                    }
    // a solve of no iterations keeps today's launches whatever the shape
    CHECK(form(ok, 0) == FirstForm::Stored && form(ok, 1) == FirstForm::FromB && form(ok, -1) == FirstForm::Stored);
    // the other members of the shape do not depend on the option
    in = ok, in.first_recompute = 0;
    const LoopShape with = loop_shape(ok), without = loop_shape(in);
    CHECK(with.ap_recomputed == without.ap_recomputed && with.fused_direction == without.fused_direction && with.b_is_p0 == without.b_is_p0 &&
          with.r0_in_ring == without.r0_in_ring && with.zero_start == without.zero_start && with.late == without.late && with.slots == without.slots);
}

static void test_default_block_rows() {
    // nobody asked: 8 for a slab without neighbours that owns its matrix, has a ring and has not switched fused_direction off
    CHECK(default_block_rows(-1, false, true, 16, 1) == 8);
    CHECK(default_block_rows(-1, false, true, 2, 1) == 8);
    CHECK(default_block_rows(-1, false, true, 16, 2) == 8);
    // each condition switched off alone: 4
    CHECK(default_block_rows(-1, true, true, 16, 1) == 4);   // neighbours
    CHECK(default_block_rows(-1, false, false, 16, 1) == 4); // a borrowed operator
    CHECK(default_block_rows(-1, false, true, 1, 1) == 4);   // the in-place form
    CHECK(default_block_rows(-1, false, true, 16, 0) == 4);  // fused_direction 0
    CHECK(default_block_rows(-1, true, false, 1, 0) == 4);
    // the environment's 0, 4 or 8 overrides on every slab
    for (int asked : {0, 4, 8})
        for (int k = 0; k < 16; ++k) CHECK(default_block_rows(asked, (k & 1) != 0, (k & 2) != 0, (k & 4) ? 16 : 1, (k & 8) ? 1 : 0) == asked);
    // any other value counts as not asked
    for (int asked : {-8, 1, 2, 3, 5, 7, 16}) {
        CHECK(default_block_rows(asked, false, true, 16, 1) == 8);
        CHECK(default_block_rows(asked, true, true, 16, 1) == 4);
    }
}

int main() {
    test_first_recomputed();
    test_default_block_rows();
    if (failures != 0) {
        std::fprintf(stderr, "first_recompute: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("first_recompute: ok\n");
    return 0;
}
