// skew_geometry.hpp -- the skewed block tiles of the r update that recomputes A p' (stencil5_block_kernels.hip, cg_update_r_recompute_kernel;
// DESIGN §9). cg_update_r_kernel leaves one r.r partial per CHUNK of 128 consecutive elements of the linear index, chunk q =
// [128 q, 128 q + 128), lane l holding the pair 2 l, 2 l + 1. A kernel that must leave the same partials and still work on blocks
// of grid rows cuts each grid row at the chunk boundaries instead of at fixed columns: tile t of grid row li is the t-th chunk that
// STARTS in that row, so a block of R grid rows is skewed by (-li n) mod 128 columns from row to row and every wave-row is exactly
// one chunk. <cstddef> only: no HIP, nothing allocates; tests/abi/skew_geometry_test.cpp walks all of it on a CPU. constexpr:
// the kernel evaluates the same functions.
#ifndef SPMV_AMD_SKEW_GEOMETRY_HPP
#define SPMV_AMD_SKEW_GEOMETRY_HPP
#include <cstddef>

namespace spmv_amd {
namespace slab {

constexpr int kChunk = 128;  // elements per chunk: one pair per lane of a wave

// the first chunk that starts in grid row li of an n-column grid (ceil(li n / 128)), and how many start there: floor(n / 128) or one
// more; none in some rows where n < 128
constexpr long long first_chunk_in_row(long long li, int n) { return (li * n + kChunk - 1) / kChunk; }
constexpr int chunks_starting_in_row(long long li, int n) { return (int)(first_chunk_in_row(li + 1, n) - first_chunk_in_row(li, n)); }
// column tiles of the skewed launch: the most chunks any grid row starts
constexpr int skew_col_tiles(int n) { return (n + kChunk - 1) / kChunk; }
// chunks of a vector of `elements` doubles that hold a pair: cg_update_r_kernel's workgroups (the odd last element rides in chunk 0)
constexpr long long chunk_count(size_t elements) {
    const size_t want = ((elements >> 1) + 63) / 64;
    return want < 1 ? 1 : (long long)want;
}

// (row block, column tile t, row r of the block) -> its chunk. exists: grid row row_block * R + r lies in the grid, starts more than
// t chunks, and the chunk holds a pair. start_col: the column of its first element. inside_row: all 128 elements lie in that grid
// row; every row's last chunk may straddle into the next row (with n < 128 every chunk does).
struct SkewChunk {
    long long chunk;
    int start_col;
    bool exists, inside_row;
};
constexpr SkewChunk skew_chunk(int row_block, int t, int r, int R, int n, int rows, long long chunks) {
    const long long li = (long long)row_block * R + r;
    const long long q = first_chunk_in_row(li, n) + t;
    const bool exists = li < rows && t < chunks_starting_in_row(li, n) && q < chunks;
    const long long start = q * kChunk - li * n;
    return SkewChunk{q, (int)start, exists, exists && start + kChunk <= n};
}

// Who owns element i of the vector: (chunk, lane, half). The odd last element of an odd-length vector belongs to no pair: lane 0 of
// chunk 0 adds it behind its own pair, as cg_update_r_kernel's thread 0 of workgroup 0 does.
struct Owner {
    long long chunk;
    int lane, half;
};
constexpr Owner owner_of(long long i) { return Owner{i / kChunk, (int)(i % kChunk) / 2, (int)(i % 2)}; }

// ---- the fused launch's block map (kernels.hpp, Stencil5Plan::block_map: one byte per block tile, row block major) ----
enum class RowBlock : unsigned char { Slow = 0, Fast = 1, Mixed = 2 };
inline RowBlock row_block_state(const unsigned char* block_map, int col_tiles, int row_block) {
    int fast = 0;
    for (int t = 0; t < col_tiles; ++t) fast += block_map[(size_t)row_block * col_tiles + t] != 0 ? 1 : 0;
    return fast == col_tiles ? RowBlock::Fast : fast == 0 ? RowBlock::Slow : RowBlock::Mixed;
}
// The recomputing r update decides per ROW BLOCK whether an element's A p' is recomputed (the fused launch did not store it) or read
// (the launch over the slow blocks stored it): every row block must be all-fast or all-slow. On the generator's matrix the slow
// ones are the 2 row blocks holding the grid's first and last grid row. out (may be null): one byte per row block, 1 = fast.
inline bool skew_eligible(const unsigned char* block_map, int row_blocks, int col_tiles, unsigned char* out = nullptr) {
    if (block_map == nullptr || row_blocks <= 0 || col_tiles <= 0) return false;
    bool ok = true;
    for (int b = 0; b < row_blocks; ++b) {
        const RowBlock state = row_block_state(block_map, col_tiles, b);
        if (state == RowBlock::Mixed) ok = false;
        if (out != nullptr) out[b] = state == RowBlock::Fast ? 1 : 0;
    }
    return ok;
}

}  // namespace slab
}  // namespace spmv_amd
#endif
