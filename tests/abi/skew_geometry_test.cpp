// Stand-alone CPU test of csrc/skew_geometry.hpp -- the skewed block tiles of the r update that recomputes A p' -- and of the decision
// that switches it on, LoopShape::ap_recomputed (csrc/slab_decisions.hpp). Grids n = 3 ... 300 with block rows R = 4 and 8: every
// element of the grid is owned by exactly one (chunk, lane, half) and every chunk by exactly one (row block, column tile, row); a
// chunk flagged "inside its grid row" really is, and one that is not flagged is not; the eligibility rule on hand-made block maps;
// the truth table written out from the rule. tests/test_ap_recompute_host.py builds it under
// -fsanitize=address,undefined and runs it; it prints "skew_geometry: ok" and returns 0, or names every check that failed.
#include <cstdio>
#include <vector>

#include "skew_geometry.hpp"
#include "slab_decisions.hpp"

using namespace spmv_amd::slab;

static int failures = 0;
static void report(int line, const char* what) {
    if (++failures <= 40) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, line, what);
}
#define CHECK(cond) ((cond) ? (void)0 : report(__LINE__, #cond))

static void test_ownership(int n, int R) {
    const long long N = (long long)n * n;
    const int rows = n, col_tiles = skew_col_tiles(n), row_blocks = (rows + R - 1) / R;
    const long long chunks = chunk_count((size_t)N), paired = 2 * (N / 2);
    CHECK(chunks == (N / 2 + 63) / 64 || (N < 2 && chunks == 1));
    std::vector<int> owned((size_t)N, 0), seen((size_t)chunks, 0);
    for (int li = 0; li < rows; ++li) {
        const int starts = chunks_starting_in_row(li, n);
        CHECK(starts == n / kChunk || starts == n / kChunk + 1);
        CHECK(starts <= col_tiles);
        CHECK(first_chunk_in_row(li, n) * kChunk >= (long long)li * n && (first_chunk_in_row(li, n) - 1) * kChunk < (long long)li * n);
    }
    for (int b = 0; b < row_blocks; ++b)
        for (int t = 0; t < col_tiles; ++t)
            for (int r = 0; r < R; ++r) {
                const SkewChunk c = skew_chunk(b, t, r, R, n, rows, chunks);
                const long long li = (long long)b * R + r;
                if (!c.exists) {
                    CHECK(!c.inside_row);
                    continue;
                }
                CHECK(li < rows && c.chunk >= 0 && c.chunk < chunks);
                if (c.chunk < 0 || c.chunk >= chunks) continue;
                ++seen[(size_t)c.chunk];
                const long long first = c.chunk * kChunk;
                CHECK(first / n == li);                       // the chunk STARTS in that grid row ...
                CHECK(c.start_col == first - li * n && c.start_col >= 0 && c.start_col < n);  // ... at this column
                CHECK(t == c.chunk - first_chunk_in_row(li, n));  // and is the t-th that does
                bool all_in_row = true;
                for (int lane = 0; lane < 64; ++lane)
                    for (int half = 0; half < 2; ++half) {
                        const long long i = first + 2 * lane + half;
                        if (i >= N || i / n != li) all_in_row = false;
                        if (i >= paired) continue;  // no pair there (the vector's end; the odd last element rides in chunk 0)
                        ++owned[(size_t)i];
                        const Owner o = owner_of(i);
                        CHECK(o.chunk == c.chunk && o.lane == lane && o.half == half);
                    }
                CHECK(c.inside_row == all_in_row);
                if (n < kChunk) CHECK(!c.inside_row);  // a row shorter than a chunk holds none
            }
    for (long long i = 0; i < paired; ++i) CHECK(owned[(size_t)i] == 1);
    if (N & 1) CHECK(owned[(size_t)(N - 1)] == 0 && seen[0] == 1);  // the odd last element: no pair; chunk 0 exists and takes it
    for (long long q = 0; q < chunks; ++q) CHECK(seen[(size_t)q] == 1);
}

static void test_eligibility() {
    const int col_tiles = 5, row_blocks = 7;
    std::vector<unsigned char> map((size_t)col_tiles * row_blocks, 1), fast((size_t)row_blocks, 9);
    // the generator's matrix: the row blocks holding the grid's first and last grid row are slow, every other one fast
    for (int t = 0; t < col_tiles; ++t) map[(size_t)t] = map[(size_t)(row_blocks - 1) * col_tiles + t] = 0;
    CHECK(skew_eligible(map.data(), row_blocks, col_tiles, fast.data()));
    for (int b = 0; b < row_blocks; ++b) {
        CHECK(fast[(size_t)b] == (b > 0 && b < row_blocks - 1 ? 1 : 0));
        CHECK(row_block_state(map.data(), col_tiles, b) == (b > 0 && b < row_blocks - 1 ? RowBlock::Fast : RowBlock::Slow));
    }
    CHECK(skew_eligible(map.data(), row_blocks, col_tiles));  // without the output array
    // one slow block tile in a fast row block, at either end and inside: mixed, not eligible
    for (int t : {0, 2, col_tiles - 1}) {
        std::vector<unsigned char> mixed = map;
        mixed[(size_t)3 * col_tiles + t] = 0;
        CHECK(row_block_state(mixed.data(), col_tiles, 3) == RowBlock::Mixed);
        CHECK(!skew_eligible(mixed.data(), row_blocks, col_tiles, fast.data()));
        CHECK(fast[3] == 0 && fast[2] == 1);  // the array is still filled: a mixed block is not fast
    }
    // one fast block tile in a slow row block
    std::vector<unsigned char> lone = map;
    lone[1] = 1;
    CHECK(!skew_eligible(lone.data(), row_blocks, col_tiles));
    // a whole row block slow in the middle, and a map without any fast block: eligible (nothing is recomputed there)
    std::vector<unsigned char> hole = map;
    for (int t = 0; t < col_tiles; ++t) hole[(size_t)4 * col_tiles + t] = 0;
    CHECK(skew_eligible(hole.data(), row_blocks, col_tiles, fast.data()) && fast[4] == 0 && fast[3] == 1);
    std::vector<unsigned char> none(map.size(), 0);
    CHECK(skew_eligible(none.data(), row_blocks, col_tiles));
    // any non-zero byte counts as fast; no map, no blocks: not eligible
    std::vector<unsigned char> loud(map.size(), 255);
    CHECK(skew_eligible(loud.data(), row_blocks, col_tiles, fast.data()) && fast[0] == 1);
    CHECK(!skew_eligible(nullptr, row_blocks, col_tiles) && !skew_eligible(map.data(), 0, col_tiles) && !skew_eligible(map.data(), row_blocks, 0));
}

// a slab that takes the form: one rank, owns its matrix, ring of 4, the block kernel on the whole slab with few slow blocks
static ShapeInputs eligible() {
    ShapeInputs in{};
    in.ring_slots = 4, in.n_local = 1 << 20, in.owns_matrix = true, in.reduce_scratch = true;
    in.fused_direction = 1, in.fused_dot = true, in.planes_and_classes = true, in.block_plan = true, in.slow_blocks = 4, in.block_tiles = 64;
    in.fuse_init_residual = true, in.x0_known_zero = true, in.zero_start_parts = 15, in.zero_rows_plus_zero = true;
    in.ap_recompute = 1, in.skew_eligible = true;
    return in;
}
static bool takes(const ShapeInputs& in) { return loop_shape(in).ap_recomputed; }

static void test_truth_table() {
    const ShapeInputs ok = eligible();
    ShapeInputs in = ok;
    CHECK(takes(ok) && loop_shape(ok).fused_direction);
    // the option and the geometry, each alone
    in = ok, in.ap_recompute = 0, CHECK(!takes(in) && loop_shape(in).fused_direction);
    in = ok, in.skew_eligible = false, CHECK(!takes(in) && loop_shape(in).fused_direction);
    // everything that switches the fused direction update off switches this off: neighbours, a borrowed operator, ring 1, the detail
    // timers, no block plan, too many slow blocks, the option itself
    in = ok, in.exchanges_halos = true, CHECK(!takes(in));
    in = ok, in.exchanges_halos = in.collective = in.has_prev = in.has_next = true, in.halo = 1024, CHECK(!takes(in));
    in = ok, in.owns_matrix = false, CHECK(!takes(in));
    in = ok, in.ring_slots = 1, CHECK(!takes(in));
    in = ok, in.detailed_timers = true, CHECK(!takes(in));
    in = ok, in.block_plan = false, CHECK(!takes(in));
    in = ok, in.planes_and_classes = false, CHECK(!takes(in));
    in = ok, in.fused_dot = false, CHECK(!takes(in));
    in = ok, in.slow_blocks = -1, CHECK(!takes(in));
    in = ok, in.slow_blocks = 60, CHECK(!takes(in));
    in = ok, in.slow_blocks = 60, in.fused_direction = 2, CHECK(takes(in));  // the cap lifted: still the fused loop
    in = ok, in.fused_direction = 0, CHECK(!takes(in));
    // it does not depend on how the solve starts, and nothing else of the shape depends on it
    in = ok, in.x0_known_zero = false, CHECK(takes(in));
    in = ok, in.zero_start_parts = 0, CHECK(takes(in));
    in = ok, in.zero_rows_plus_zero = false, CHECK(takes(in));
    in = ok, in.ap_recompute = 0;
    const LoopShape with = loop_shape(ok), without = loop_shape(in);
    CHECK(with.fused_direction == without.fused_direction && with.zero_start == without.zero_start && with.r0_in_ring == without.r0_in_ring &&
          with.b_is_p0 == without.b_is_p0 && with.late == without.late && with.pipeline == without.pipeline && with.slots == without.slots);
}

int main() {
    for (int n = 3; n <= 300; ++n)
        for (int R : {4, 8}) test_ownership(n, R);
    test_eligibility();
    test_truth_table();
    if (failures != 0) {
        std::fprintf(stderr, "skew_geometry: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("skew_geometry: ok\n");
    return 0;
}
