// Stand-alone CPU test of what csrc/slab_decisions.hpp decides about the first stage of a solve: LoopShape::b_is_p0 (b serves as p0
// and iteration 0's SpMV sums b.b) and the matrix fact it rests on, sums_to_plus_zero. The truth table is written out from the rule
// (DESIGN §4); the fact is checked on hand-made rows against the two summation orders the kernels use, evaluated here on zeros.
// tests/test_first_stage_host.py builds it under -fsanitize=address,undefined and runs it; it prints "slab_first_stage: ok" and
// returns 0, or names every check that failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "slab_decisions.hpp"

using namespace spmv_amd::slab;

static int failures = 0;
static void report(int line, const char* what) {
    ++failures;
    std::fprintf(stderr, "%s:%d: %s\n", __FILE__, line, what);
}
#define CHECK(cond) ((cond) ? (void)0 : report(__LINE__, #cond))

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

// a slab that takes the shape: one rank, owns its matrix, ring of 4, the block kernel on the whole slab, x0 = the library's zeros
static ShapeInputs eligible() {
    ShapeInputs in{};
    in.ring_slots = 4, in.n_local = 1 << 20, in.owns_matrix = true, in.reduce_scratch = true;
    in.fused_direction = 1, in.fused_dot = true, in.planes_and_classes = true, in.block_plan = true, in.slow_blocks = 4, in.block_tiles = 64;
    in.fuse_init_residual = true, in.x0_known_zero = true, in.zero_start_parts = 15, in.zero_rows_plus_zero = true;
    return in;
}
static bool takes(const ShapeInputs& in) { return loop_shape(in).b_is_p0; }

static void test_truth_table() {
    const ShapeInputs ok = eligible();
    ShapeInputs in = ok;
    CHECK(takes(ok));
    {
        const LoopShape L = loop_shape(ok);
        CHECK(L.zero_start && L.r0_in_ring && L.fused_direction && !L.multi && !L.detail);
    }
    // each precondition switched off alone
    in = ok, in.x0_known_zero = false, CHECK(!takes(in));       // x0 uploaded by the caller, zeros or not
    in = ok, in.zero_rows_plus_zero = false, CHECK(!takes(in)); // a row of the matrix may sum to -0.0 or NaN
    in = ok, in.fused_dot = false, CHECK(!takes(in));
    in = ok, in.planes_and_classes = false, CHECK(!takes(in));  // the launches are the one-row kernel's
    in = ok, in.block_plan = false, CHECK(!takes(in));
    in = ok, in.fuse_init_residual = false, CHECK(!takes(in));
    in = ok, in.detailed_timers = true, CHECK(!takes(in));
    // the part bits: 8 alone is not enough (it sits on top of 1 and 2), 7 is the shape of before, 4 is not needed
    in = ok, in.zero_start_parts = 7, CHECK(!takes(in));
    in = ok, in.zero_start_parts = 8, CHECK(!takes(in));
    in = ok, in.zero_start_parts = 9, CHECK(!takes(in));
    in = ok, in.zero_start_parts = 10, CHECK(!takes(in));
    in = ok, in.zero_start_parts = 11, CHECK(takes(in));
    in = ok, in.zero_start_parts = 15, CHECK(takes(in));
    in = ok, in.zero_start_parts = 0, CHECK(!takes(in));         // zero_start off: the mask is 0
    // neighbours, ring 1, a borrowed operator: exactly like zero_start
    in = ok, in.exchanges_halos = true, CHECK(!takes(in));
    in = ok, in.exchanges_halos = in.collective = in.has_prev = in.has_next = true, in.halo = 1024, CHECK(!takes(in));
    in = ok, in.ring_slots = 1, CHECK(!takes(in));
    in = ok, in.owns_matrix = false, CHECK(!takes(in));
    // it does not depend on the direction update's form, nor on the slow blocks' share
    in = ok, in.fused_direction = 0, CHECK(takes(in) && !loop_shape(in).fused_direction);
    in = ok, in.slow_blocks = 64, CHECK(takes(in) && !loop_shape(in).fused_direction);
    // and the other members of the shape do not depend on it
    in = ok, in.zero_start_parts = 7;
    const LoopShape with = loop_shape(ok), without = loop_shape(in);
    CHECK(with.zero_start == without.zero_start && with.r0_in_ring == without.r0_in_ring && with.fused_direction == without.fused_direction &&
          with.late == without.late && with.pipeline == without.pipeline && with.slots == without.slots);
    CHECK(flush_skips_x0(true, 15) && flush_skips_x0(true, 12) && !flush_skips_x0(true, 11));
}

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}
// The two orders the kernels evaluate a row in, on zero operands (stencil_row_device.hpp): the interior chain starts from the
// first product, the CSR loop from 0.0.
static double chain_from_first_product(const std::vector<double>& c) {
    double sum = c[0] * 0.0;
    for (size_t k = 1; k < c.size(); ++k) sum = std::fma(c[k], 0.0, sum);
    return sum;
}
static double chain_from_zero(const std::vector<double>& c) {
    double sum = 0.0;
    for (double v : c) sum = std::fma(v, 0.0, sum);
    return sum;
}
static bool rule(const std::vector<double>& c) { return sums_to_plus_zero(c.data(), (int)c.size()); }

static void test_rows() {
    const uint64_t plus_zero = bits(0.0), minus_zero = bits(-0.0);
    CHECK(plus_zero != minus_zero);
    // whatever the rule accepts sums to +0.0 in both orders and in every rotation of the row
    const std::vector<std::vector<double>> accepted = {
        {-1.0, 5.0, -1.0, -1.0, -1.0},  // the generator's quintuple (W, C, E, N, S)
        {-1.0, -1.0, 5.0, -1.0},        // an edge column's four entries
        {-1.0, 5.0, -1.0},              // a corner of the grid
        {-1.0, -2.0, 0.0, -3.0, -4.0},  // one +0.0 among negatives
        {-0.0, -0.0, 4.9e-324, -0.0, -0.0},  // one positive subnormal
        {1.7976931348623157e308, -1.7976931348623157e308, -1.0, -0.0, -5.0},
    };
    for (const std::vector<double>& row : accepted) {
        CHECK(rule(row));
        std::vector<double> r = row;
        for (size_t turn = 0; turn < row.size(); ++turn) {
            CHECK(bits(chain_from_first_product(r)) == plus_zero && bits(chain_from_zero(r)) == plus_zero);
            r.push_back(r.front()), r.erase(r.begin());
        }
    }
    // all negative: the chain from the first product gives -0.0, and fma(-1, -0.0, b) turns b = -0.0 into +0.0
    const std::vector<double> negative = {-1.0, -5.0, -1.0, -1.0, -1.0};
    CHECK(!rule(negative) && bits(chain_from_first_product(negative)) == minus_zero);
    CHECK(bits(std::fma(-1.0, chain_from_first_product(negative), -0.0)) == plus_zero);
    // a single -0.0 coefficient, and a row of them
    CHECK(!rule({-0.0}) && !rule({-0.0, -0.0, -0.0, -0.0, -0.0}) && bits(chain_from_first_product({-0.0, -0.0})) == minus_zero);
    // the conservative side: a chain from 0.0 would still give +0.0 there; the rule does not look at the order
    CHECK(bits(chain_from_zero(negative)) == plus_zero && !rule(negative));
    // an infinity or a NaN anywhere: inf x 0 = NaN
    CHECK(!rule({-1.0, kInf, -1.0, -1.0, -1.0}) && std::isnan(chain_from_zero({-1.0, kInf, -1.0, -1.0, -1.0})));
    CHECK(!rule({-1.0, 5.0, -kInf, -1.0, -1.0}) && !rule({kNaN, 5.0, -1.0, -1.0, -1.0}) && !rule({-1.0, 5.0, -1.0, -1.0, -kNaN}));
    CHECK(!rule({}));  // no coefficient: nothing has its sign bit clear
    // the two pieces
    CHECK(finite_value(0.0) && finite_value(-0.0) && finite_value(-1.7976931348623157e308) && finite_value(4.9e-324) && !finite_value(kInf) &&
          !finite_value(-kInf) && !finite_value(kNaN));
    CHECK(sign_bit_clear(0.0) && !sign_bit_clear(-0.0) && sign_bit_clear(4.9e-324) && !sign_bit_clear(-4.9e-324) && sign_bit_clear(3.0) && !sign_bit_clear(-3.0));
}

int main() {
    test_truth_table();
    test_rows();
    if (failures != 0) {
        std::fprintf(stderr, "slab_first_stage: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("slab_first_stage: ok\n");
    return 0;
}
