// kernels.hpp -- host-callable launchers of the HIP kernels (gfx950 only).
// Every launcher enqueues on the given stream and returns; none synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

struct PeerMailbox;  // comm.hpp: the dot products' all-reduce as stores between the GPUs

namespace spmv_amd {

// A row slab of a CSR matrix resident in HBM. For a single-GPU operator the slab
// is the whole matrix (row_offset = 0, nnz_base = 0, no halos).
struct SlabCsr {
    const int* row_ptr = nullptr;    // n_local + 1 entries, rebased so row_ptr[0] == 0
    const int* col_idx = nullptr;    // GLOBAL column indices
    const double* values = nullptr;
    int n_local = 0;                 // rows in the slab
    int row_offset = 0;              // global index of local row 0
    long long nnz_local = 0;
    int max_row_nnz = 0;             // longest row of the slab (0 = not known): steers csr_auto_variant
    long long nnz_base = 0;          // global CSR position of the slab's first entry
    int n_global = 0;                // rows of the whole matrix
    int grid_size = -1;              // n of the n x n stencil, <= 0 if not a stencil
    bool verified_stencil = false;   // structure checked against the complete 5-point pattern
    // x is addressed as x[col - row_offset]; indices in [-halo_before, n_local + halo_after)
    // are readable, anything else contributes 0 (reference halo kernel semantics).
    int halo_before = 0;
    int halo_after = 0;
};

// Launch switches (SPMV_AMD_* environment variables, tools/README.md). They are read ONCE, when an operator is initialised or
// a solver slab is created (current_launch_shape()), into this struct; nothing on a launch path calls getenv.
struct Tunables {
    int rowlds_min_grid = 512;    // SPMV_AMD_ROWLDS_MIN_GRID: smallest grid that takes row-lds automatically (tests force it down)
    int rowlds_group = 0;         // SPMV_AMD_ROWLDS_GROUP: consecutive row-lds tiles per XCD; 0 = derived from the grid (xcd_run_group())
    // SPMV_AMD_ROWLDS_BLOCK_ROWS: grid rows per wave of a solver slab's in-loop SpMV (block tiles): 0 (the one-row kernel), 4 or 8.
    // 20 000^2 on MI355X, one process, alternated: 1.636 ms / 1.064 / 1.086 (profiles/r13_block_rows_ab.txt). With the direction
    // update inside the SpMV (DirectionSpmv) 8 makes that launch 2 % shorter, and with A p' recomputed by the r update a whole solve
    // 0.5 ms shorter (profiles/r23_ap_recompute_ab.txt, r24_first_recompute_ab.txt): a solver slab on which that loop can run takes 8
    // where the variable is unset (slab_decisions.hpp, default_block_rows); operators and every other slab keep 4.
    int rowlds_block_rows = 4;
    // SPMV_AMD_STENCIL7_ROWLDS_MIN_GRID: smallest n of an n^3 grid that takes stencil7/row-lds automatically. Measured on MI355X
    // (profiles/r18_stencil7_bench.txt), row-lds / row-direct medians: 64^3 7.9 / 9.9 us, 96^3 20.3 / 24.0, 128^3 38.4 / 40.9,
    // 160^3 80.8 / 83.6, 256^3 225 / 287: row-lds is faster from the smallest size measured on
    int stencil7_rowlds_min_grid = 64;
};

// How many consecutive logical blocks (each `block_columns` grid columns wide) one XCD takes of every run of
// 8 * group, for kernels that walk an n x n grid row-major. Measured on MI355X (profiles/r02_xcd_group.txt): the
// best run is one grid row plus ~1100 columns -- STENCIL5 row-lds at 20 000^2: 3.74-3.79 ms with runs of 4 tiles per
// XCD, 3.65-3.71 ms with 21; 17 000^2: 2.77 -> 2.70 ms; stencil-aware ELLPACK at 20 000^2: 4.01 ms in dispatch
// order, 3.6-3.7 ms so -- for grids of 8192 columns and more; smaller grids keep short runs (4096^2: 0.150 vs 0.165 ms).
inline int xcd_run_group(int n, int block_columns, int small_grid_group) {
    if (n < 8000) return small_grid_group;
    const int g = (n + 1100 + 8 * block_columns - 1) / (8 * block_columns);
    return g < 1 ? 1 : (g > 64 ? 64 : g);
}

struct LaunchShape {
    Tunables knobs;
    // walk the tiles from the last to the first (row-lds kernel): results are identical, only the order in
    // which addresses are touched changes (sweep direction alternation of the CG loop, cg_slab.hip)
    bool reverse = false;
};

// ---- structure ----
// Fills row_ptr/col_idx/values of the slab [row_offset, row_offset+n_local) of the
// n x n 5-point stencil (centre/off values as given), rows sorted by column.
void launch_generate_stencil5_csr(int n, int row_offset, int n_local, long long nnz_base,
                                  double center, double off, int* row_ptr, int* col_idx,
                                  double* values, hipStream_t stream);
// Sets *d_mismatch (int, zeroed by the caller) to non-zero if any row of the slab deviates
// from the complete 5-point pattern of an n x n grid.
void launch_verify_stencil5_csr(const SlabCsr& m, int* d_mismatch, hipStream_t stream);

// ---- STENCIL5 SpMV ----
// y[r] = alpha * (A x)[r]. d_dot_partials, if non-null, receives one partial of
// sum_r x[r]*y_unscaled[r] per launched wave (count: stencil5_partials_needed()).
enum class Stencil5Variant { Auto, RowDirect, RowGeneric, RowLds };
// Everything about one STENCIL5 launch over local rows [first_row, last_row) that does not depend on the vectors:
// which kernel, its grid, how many dot partials it writes. Computed once per (slab, row range) -- by an operator's
// init, by a solver slab's creation -- and reused for every launch.
struct Stencil5Plan {
    Stencil5Variant variant = Stencil5Variant::RowGeneric;
    int first_row = 0, last_row = 0;
    int gi_lo = 0, gi_hi = 0;  // row-direct / row-lds: the local grid rows of the range
    int row_blocks = 0;        // row-generic: workgroups of the launch; row-direct / row-lds: workgroups per grid row
    int xcd_run = 0;           // row-lds: consecutive tiles (block tiles, where the launch takes them) one XCD takes of every run of 8 * xcd_run
    // row-lds: grid rows per block tile of the in-loop SpMV (0, 4 or 8; Tunables) and the range's block map -- one byte per block
    // tile, 1 = all its tiles uniform and all its rows present (launch_block_map; device memory of the plan's owner). Without a
    // map the launch is the one-row kernel's.
    int block_rows = 0;
    const unsigned char* block_map = nullptr;
    int partials = 0;          // dot-partial slots one launch writes (a fixed function of the slab and the range)
    const char* name = "";     // "stencil5/row-lds", ...
};
Stencil5Plan plan_stencil5(const SlabCsr& m, int first_row, int last_row, Stencil5Variant variant,
                           const LaunchShape& shape);
int rowlds_xcd_run_rule(int n);  // the untuned run length of row-lds tiles per XCD for an n x n grid
// The first SpMV of a CG solve fused with the initial residual (row-lds plans only): instead of storing y = A x the
// launch writes r = b - A x and p = r and one partial of r.r per wave into d_dot_partials.
// r == nullptr: the value is stored once, as p (the caller reads r0 from there).
struct ResidualOut {
    const double* b;
    double* r;
    double* p;
};
// The symmetric coefficient form of a solver slab (cg_slab.hip): a 5-point stencil whose W and N entries equal, bit for bit, the
// E entry of row i-1 and the S entry of row i-n needs only C, E and S per row. ce = [C, E] of local row lr at ce[2 lr], ce[2 lr + 1]
// (E = 0 in column n-1); s = S of local row lr at s[lr] (0 in the grid's last row), with ONE grid row of halo in front of it:
// s[lr - n], lr < n, is the slab's own N entry of local row lr (0 in the grid's first row). The row-lds kernel then streams 24 B
// of coefficients per row instead of 40, with the same fma chains. Row-lds launches only; a null view = the CSR form.
//
// Tile classes (a property inside this form): a row-lds tile -- 128 columns of one grid row -- of global grid rows 1 .. n-2 is
// UNIFORM when every coefficient its fma chains multiply equals, as a 64-bit pattern, the matching member of one slab-wide
// quintuple (w, c, e, n, s): interior columns W, C, E, N, S; column 0 N, C, E, S; column n-1 N, W, C, S. `cls` holds one byte per
// tile at [local grid row * col_tiles + col_tile] (1 = uniform, 0 = stream the planes), written once at creation from the CSR
// values (launch_classify_tiles). A wave on a uniform tile loads no coefficient at all and runs the same fma chains on the
// quintuple, which travels as launch arguments. cls == nullptr: every tile streams the planes.
struct SymPlanes {
    const double* ce = nullptr;  // 16-byte aligned
    const double* s = nullptr;
    const unsigned char* cls = nullptr;
    double w = 0.0, c = 0.0, e = 0.0, n = 0.0, s5 = 0.0;  // the quintuple (s5: S)
};
// Fills the planes from a slab that passed verify_stencil (s: the local part, halo in front).
void launch_fill_sym_planes(const SlabCsr& m, double* ce, double* s, hipStream_t stream);
// Writes the tile class map of a verified stencil slab made of whole grid rows (SymPlanes: one byte per tile, local grid rows x
// ceil(n / 128) of them; the grid's first and last grid row get 0) by comparing the CSR values with `quintuple` = {W, C, E, N, S}
// bit for bit, and adds the number of uniform tiles to *d_uniform (zeroed by the caller).
void launch_classify_tiles(const SlabCsr& m, const double quintuple[5], unsigned char* cls, unsigned long long* d_uniform, hipStream_t stream);
// One Chebyshev step fused into a row-lds launch (kMode 3; precond.hip): with w = A z kept in registers,
//   t = fma(-1.0, w, r) ; u = dinv * t ; d = fma(g, u, h * d) ; z_out = z + d
// d is updated in place (its own lane only), z_out is a SECOND vector (neighbouring tiles still read z). last != 0: the launch also
// writes one partial of r . z_out per wave, in the slot layout of the p.Ap partials. work_count (may be null): incremented once per
// launch that was not skipped.
struct ChebStep {
    const double* r = nullptr;
    const double* dinv = nullptr;
    double* d = nullptr;
    double* z_out = nullptr;
    double g = 0.0, h = 0.0;
    int last = 0;
    int* work_count = nullptr;
};
int rowlds_col_tiles(int n);  // row-lds tiles per grid row
// Block tiles of a row-lds plan -- 128 columns x plan.block_rows grid rows, the last block of the range may be short -- (0: none)
// and its block map, written from the slab's class map (`cls`: SymPlanes): out[row block * tiles per grid row + column tile].
int rowlds_block_tiles(const Stencil5Plan& plan);
void launch_block_map(const unsigned char* cls, const Stencil5Plan& plan, unsigned char* out, hipStream_t stream);
// Sets *d_mismatch (int, zeroed by the caller) if any value the row-lds kernel would take from the planes in grid rows 1 .. n-2
// (W = E[i-1], N = S[i-n] or the halo row, C, E, S) differs in its 64-bit pattern from the CSR entry it stands for.
void launch_verify_sym_planes(const SlabCsr& m, const SymPlanes& planes, int* d_mismatch, hipStream_t stream);

// Launch by plan. reverse: walk the tiles from the last to the first (row-lds only; same results).
// init (may be null): see ResidualOut; y is then not written and may be null.
// planes (may be null; row-lds plans only): the symmetric coefficient form.
// A row-lds plan with a block map (Stencil5Plan) takes block tiles -- stencil5_rowlds_block_kernel, the same rows and partial slots --
// when the launch wants dot partials, has no `init` and `planes` carries a class map; every other launch is the one-row kernel's.
// x_zero (with `init`, row-lds plans, slabs without halo rows): the caller knows that x holds +0.0 in every element. The launch then
// requests no x value on grid rows 1 .. n-2 -- the five operands are 0.0 in registers and the same chains run on them, so signed
// zeros and the NaN of an infinite coefficient come out as they did -- and reads x only on the grid's first and last grid row.
// ap_not_stored (block-tile launches only; anything else is an error): y is left alone on the fast blocks, the partials are written
// as ever -- launch_cg_update_r_recompute follows (LoopShape::first_recomputed).
int launch_stencil5_spmv(const SlabCsr& m, const Stencil5Plan& plan, const double* x, double* y, double alpha,
                         double* d_dot_partials, const int* d_skip_flag, bool reverse, hipStream_t stream,
                         const ResidualOut* init = nullptr, const SymPlanes* planes = nullptr, bool x_zero = false, bool ap_not_stored = false);
// The block-tile launch that launch_stencil5_spmv hands such a plan to (stencil5_block_kernels.hip); callers go through it.
void launch_rowlds_block(const SlabCsr& m, const Stencil5Plan& plan, const double* x, double* y, double alpha, double* d_dot_partials,
                         const int* d_skip_flag, bool reverse, hipStream_t stream, const SymPlanes& planes, bool ap_not_stored);
// The CG direction update inside the in-loop block SpMV (stencil5_direction_block_kernel; slabs without neighbours whose plan has
// a block map): p_out = direction(r, s->beta, p_in), y = alpha A p_out and the p_out . (A p_out) partials of the plan's slots, in one
// launch over the block tiles plus one over `slow_list` -- the indices of the range's block tiles whose map byte is 0 (device
// memory, slow_count of them), which the first launch only writes p_out for. Both launches return on the scalars unless
// s->iterations == iteration and s->converged == 0. Returns the partial slots written (the plan's).
struct CgScalars;
struct DirectionSpmv {
    const CgScalars* s;
    int iteration;
    bool fma_form;
    const double* r;
    const double* p_in;
    double* p_out;
    const int* slow_list;
    int slow_count;
    bool ap_not_stored = false;  // the first launch leaves y alone on its fast blocks: launch_cg_update_r_recompute follows
};
int launch_stencil5_direction_spmv(const SlabCsr& m, const Stencil5Plan& plan, const DirectionSpmv& d, double* y, double alpha,
                                   double* d_dot_partials, bool reverse, hipStream_t stream, const SymPlanes& planes);
// r -= (s->rr_old / s->pAp) A p_new with the r.r partials of launch_cg_update_r (same slots, same bits; returns their count), behind
// a launch_stencil5_direction_spmv with ap_not_stored: A p_new is recomputed from p_new on the skewed block tiles of
// skew_geometry.hpp where the element's row block is fast (row_fast: one byte per row block of the plan's block map, 1 = every
// block tile fast, 0 = none; slab::skew_eligible) and read from Ap elsewhere. The whole-slab plan of a slab without halo rows.
// r_is_p (iteration 0, where r0 and p0 are one vector: b, or ring slot 0): the out-of-place instance, r = p_new - alpha A p_new with
// launch_cg_update_r_from's bits; r is only written, p_new only read.
int launch_cg_update_r_recompute(const SlabCsr& m, const Stencil5Plan& plan, const CgScalars* s, const double* p_new, const double* Ap, double* r,
                                 double* partials, const unsigned char* row_fast, bool reverse, hipStream_t stream, const SymPlanes& planes,
                                 bool r_is_p = false);
// Iteration 0's SpMV of a solve that starts from x0 = 0 on a matrix whose rows sum to +0.0 over zero operands (slab_decisions.hpp,
// LoopShape::b_is_p0; stencil5_first_block_kernel): the in-loop block launch on x = b -- y = alpha A b and the b . (A b) partials,
// as launch_stencil5_spmv writes them -- that also leaves the b . b partials in `self_partials`, same slots, each summed as the
// launch of the initial residual sums r0 . r0 (r0 is b bit for bit there). Slabs without halo rows whose plan has a block map.
// Returns the partial slots written to each array (the plan's). ap_not_stored: as in launch_stencil5_spmv.
int launch_stencil5_first_spmv(const SlabCsr& m, const Stencil5Plan& plan, const double* b, double* y, double alpha, double* d_dot_partials,
                               double* self_partials, bool reverse, hipStream_t stream, const SymPlanes& planes, bool ap_not_stored = false);
// Sets *d_bad (int, zeroed by the caller) if any local row's stored coefficients fail slab_decisions.hpp's sums_to_plus_zero.
void launch_rows_plus_zero(const SlabCsr& m, int* d_bad, hipStream_t stream);
// The fused Chebyshev step over a row-lds plan (ChebStep): z is read as the SpMV's x, A z is not written. Returns the partial slots
// a last step writes (the plan's), or -1 without launching when the plan is not a row-lds one.
int launch_stencil5_cheb_step(const SlabCsr& m, const Stencil5Plan& plan, const double* z, const ChebStep& step, double* d_dot_partials,
                              const int* d_skip_flag, hipStream_t stream);
// first_row/last_row restrict the launch to local rows [first_row, last_row); used to split
// interior rows from halo-dependent rows. Returns the number of dot partials written (0 when
// d_dot_partials is null).
int launch_stencil5_spmv(const SlabCsr& m, const double* x, double* y, double alpha,
                          int first_row, int last_row, double* d_dot_partials,
                          const int* d_skip_flag, Stencil5Variant variant,
                          const LaunchShape& shape, hipStream_t stream);

// The first and the last grid row of a slab made of whole grid rows (the rows that wait for the halos), in one
// launch where the row-lds kernel applies, in two otherwise. Partial slots: first grid row's, then last grid row's.
// `head` / `tail` = the plans of the slab's first / last grid row.
int launch_stencil5_spmv_first_and_last_gridrow(const SlabCsr& m, const Stencil5Plan& head, const Stencil5Plan& tail, const double* x,
                                                double* y, double alpha, double* d_dot_partials, const int* d_skip_flag,
                                                hipStream_t stream, const ResidualOut* init = nullptr, const SymPlanes* planes = nullptr);

// ---- CSR SpMV ----
enum class CsrVariant { Auto, Stream, Adaptive, RowScalar, Wavefront };
CsrVariant csr_auto_variant(const SlabCsr& m);
// d_dot_partials (may be null; stream / adaptive variants of SQUARE matrices only): one partial of x . (A x) per logical block,
// csr_fused_dot_partials() of them (0 = the variant has no fused form).
void launch_csr_spmv(const SlabCsr& m, const double* x, double* y, double alpha,
                     CsrVariant variant, hipStream_t stream, double* d_dot_partials = nullptr);
int csr_fused_dot_partials(const SlabCsr& m, CsrVariant variant);

// ---- STENCIL7 (n x n x n 7-point stencil in CSR form; stencil7_kernels.hip) ----
// The 3-D geometry travels beside the view: SlabCsr::grid_size / verified_stencil mean "2-D 5-point" and stay unset here.
// Fills the CSR of the whole n^3 generator matrix, rows sorted by column ([D,N,W,C,E,S,U] minus the absent ones).
void launch_generate_stencil7_csr(int n, double center, double off, int* row_ptr, int* col_idx, double* values, hipStream_t stream);
// Sets *d_mismatch (int, zeroed by the caller) if any row deviates from the complete 7-point pattern of an n^3 grid. The caller has
// checked m.n_local == n^3 and m.nnz_local == 7 n^3 - 6 n^2 (the analytic offsets then stay inside the arrays).
void launch_verify_stencil7_csr(const SlabCsr& m, int n, int* d_mismatch, hipStream_t stream);
enum class Stencil7Variant { Auto, RowLds, RowDirect, CsrLoop };
// One launch over the whole matrix, computed once per init / variant change. CsrLoop (unverified matrices, n < 2) is the CSR
// launcher's Auto variant; its partials are csr_fused_dot_partials() (0 = no fused form).
struct Stencil7Plan {
    Stencil7Variant variant = Stencil7Variant::CsrLoop;
    int n = 0;           // the grid (row-lds / row-direct)
    int col_blocks = 0;  // row-lds: 128-column tiles per grid row; row-direct: 256-column blocks
    int xcd_run = 1;     // row-lds: consecutive tiles one XCD takes of every run of 8 * xcd_run
    int partials = 0;    // dot-partial slots a launch with partials writes
    const char* name = "stencil7/csr-loop";
};
int stencil7_xcd_run_rule(int n);
Stencil7Plan plan_stencil7(const SlabCsr& m, int n, bool verified, Stencil7Variant want, const Tunables& knobs);
// y = alpha A x. d_dot_partials (may be null): the partials of x . (A x), unscaled, p.partials of them -- row-lds / row-direct in
// the shapes of tests/reduction_restatement.py's rowlds_partials / rowdirect_partials over n^2 grid rows of n columns.
// d_skip_flag (may be null; row-lds / row-direct): nothing is read or written once it is set. reverse: tiles walked last to first,
// same bits, same slots. Returns the partial slots written.
int launch_stencil7_spmv(const SlabCsr& m, const Stencil7Plan& p, const double* x, double* y, double alpha, double* d_dot_partials,
                         const int* d_skip_flag, bool reverse, hipStream_t stream);

// ---- ELLPACK SpMV (device layout: slot-major, element (r,k) at [k * rows + r]) ----
void launch_ell_transpose(int rows, int width, const int* idx_rowmajor, const double* val_rowmajor,
                          int* idx_slotmajor, double* val_slotmajor, hipStream_t stream);
// grid_hint: n if the matrix is known to be an n x n stencil (block -> XCD relabelling is sized to a grid row), else 0.
void launch_ell_spmv(int rows, int width, const int* idx, const double* val, const double* x,
                     double* y, double alpha, double beta, hipStream_t stream,
                     int grid_hint = 0, double* d_dot_partials = nullptr);
// d_dot_partials (may be null; square matrices): one partial of x . (A x) per workgroup, ell_fused_dot_partials() of them.
int ell_fused_dot_partials(int rows);
// Interior rows take W,C,E,N,S from slots 1,2,3,0,4 with computed columns; others walk slots.
void launch_ell_stencil5_spmv(int rows, int width, int grid_size, const int* idx,
                              const double* val, const double* x, double* y, double alpha,
                              double beta, hipStream_t stream, double* d_dot_partials = nullptr);

// ---- BLAS1 + reductions for CG ----
// Device scalars of one CG solve, laid out in one small allocation.
struct CgScalars {
    double rr_old;
    double rr_new;
    double pAp;
    double b_norm;
    double residual;
    double alpha;
    double beta;
    int converged;
    int iterations;
    int max_history;
    int stop_at;  // LAB build only (read through cg_stop_at(), reduce_device.hpp; the product library ignores the field): the scalar
                  // step of this iteration declares convergence whatever the residual, so that a stand-in slab (whose mirrored
                  // system does not converge in 14 iterations) does a converging solve's work: 0 = off
    // r.r after step k in slot k & 1 (slot 0: the initial r.r): a launch that holds step k AND work that needs beta_k reads
    // beta_k = rr_new / rr_ring[(k - 1) & 1] in every workgroup without waiting for the step -- the step writes the OTHER slot
    // (and rr_old, which only later launches read)
    double rr_ring[2];
};

void launch_fill(double* d, size_t n, double value, hipStream_t stream);
// y = y + a*x   (reference axpy_kernel, cg_solver.cu:38-43)
void launch_axpy(size_t n, double a, const double* x, double* y, hipStream_t stream);
// z = a*x + b*y (reference axpby_kernel, cg_solver.cu:48-54)
void launch_axpby(size_t n, double a, const double* x, double b, const double* y, double* z,
                  hipStream_t stream);
// y += (*d_a)*x ; y -= (*d_a)*x ; p = r + (*d_b)*p (cg_solver.cu:59-95)
void launch_axpy_dev(size_t n, const double* d_a, const double* x, double* y, bool subtract,
                     hipStream_t stream);
void launch_update_p_dev(size_t n, const double* r, const double* d_b, double* p,
                         hipStream_t stream);
// result = sum x[i]*y[i], fixed reduction shape (deterministic run to run). scratch must
// hold dot_scratch_doubles(n) doubles and be zeroed once after allocation (ticket counter).
size_t dot_scratch_doubles(size_t n);
// The grid of every streaming kernel (one-wave workgroups, one 16-byte pair per lane) = the partials a reducing one writes.
unsigned stream_grid(size_t n);
// The first half of launch_dot alone: partials[block] of x.y, stream_grid(n) of them.
void launch_dot_partials(size_t n, const double* x, const double* y, double* partials, hipStream_t stream);
void launch_dot(size_t n, const double* x, const double* y, double* scratch, double* d_result,
                hipStream_t stream);
// *d_out = (*d_num) / (*d_den)   (scalar_divide_kernel, cg_solver.cu:414-419)
void launch_scalar_divide(const double* d_num, const double* d_den, double* d_out,
                          hipStream_t stream);
// check_convergence_kernel (cg_solver.cu:424-431)
void launch_check_convergence(const double* d_rr_new, double b_norm, double tol, int* d_converged,
                              double* d_residual, hipStream_t stream);

// ---- reductions of the CG loop ----
// Scratch of the reductions of ONE stream (slice sums, boundary-row extras, ticket; reduce_device.hpp): reduce_scratch_doubles()
// doubles, zero before the first use (every reduction leaves it ready for the next).
struct ReduceScratch {
    double* base = nullptr;  // null: a single workgroup sums everything (short lists only)
};
int reduce_scratch_doubles();
double* reduce_scratch_alloc();  // uncached device memory where the runtime offers it, zeroed; hipFree releases it

// Device-side arrival flag of a halo exchange (round 5): instead of a cross-stream event wait in front of the launch that reads
// the halo rows, the side stream raises *flag to the exchange's sequence number behind the receive (launch_halo_arrived) and the
// boundary waves of launch_stencil5_edges_and_reduce wait for it themselves -- bounded by timeout_ticks of the 100 MHz wall
// clock; a wave that gives up sets *late (host-coherent pinned memory), which ends the run on the host. flag == nullptr: none.
struct HaloArrival {
    const unsigned* flag = nullptr;
    unsigned expected = 0;
    long long timeout_ticks = 0;
    int* late = nullptr;
};
void launch_halo_arrived(unsigned* d_flag, unsigned sequence, hipStream_t stream);

// The first and / or last grid row of a solver slab (the rows that wait for the halos) AND the reduction of the SpMV's p.Ap
// partials -- the interior launch's d_interior_partials plus these rows' own -- into *d_out, in ONE launch (spmv_kernels.hip).
// `interior` = the plan of the launch over the other rows. Returns false, having launched nothing, where the fused form does
// not apply (not a row-lds slab, a slab of fewer than three grid rows): the caller then
// launches the rows and the reduction separately.
bool launch_stencil5_edges_and_reduce(const SlabCsr& m, const Stencil5Plan& interior, bool first_gridrow, bool last_gridrow, const double* x,
                                      double* y, double alpha, const double* d_interior_partials, double* d_out, const int* d_skip_flag,
                                      const ReduceScratch& scratch, int* host_progress, int progress_value, const PeerMailbox* mailbox,
                                      hipStream_t stream, const HaloArrival& halo = HaloArrival{}, const SymPlanes* planes = nullptr);

// ---- fused CG steps of the slab solver (all skip their work when s->converged) ----
// r = b - Ap ; p = r ; partials of r.r
void launch_cg_init_residual(size_t n, const double* b, const double* Ap, double* r, double* p,
                             double* partials, hipStream_t stream);
// alpha = rr_old / pAp (per thread, from the scalars) ; r -= alpha Ap ; partials of r.r
// reverse: workgroups walk the vectors from the end (same results, same partial slots).
void launch_cg_update_r(size_t n, const CgScalars* s, const double* Ap, double* r, double* partials,
                        hipStream_t stream, bool reverse = false);
// The same out of place: r_out = r_in - alpha Ap, same partials (iteration 0 of a solve whose r0 lies in the direction ring alone).
void launch_cg_update_r_from(size_t n, const CgScalars* s, const double* Ap, const double* r_in, double* r_out, double* partials,
                             hipStream_t stream, bool reverse = false);
// x += alpha p (the update of iteration `iteration`), then p = 1.0*r + beta*p unless that iteration
// converged; one pass over p (axpy + axpby of cg_solver_mgpu_partitioned.cu:598,682 fused).
// x = x_in + alpha p: x_in is x, or the stored initial guess in the first iteration of a solve.
// fma_form: p = fma(beta, p, r) (the single-GPU device solver's update_p_kernel, cg_solver.cu:90-95) instead of
// fma(1.0, r, beta*p) (the multi-GPU solver's axpby_kernel, mgpu :136-140).
void launch_cg_update_px(size_t n, const CgScalars* s, const double* r, double* p, const double* x_in,
                         double* x, int iteration, hipStream_t stream, bool reverse = false, bool fma_form = false);
// ---- deferred x update (cg_slab.hip, "direction ring") ----
// p_out = 1.0*r + beta*p_in for iteration `iteration` unless it converged: the direction update written out
// of place, so that p_in stays available for a later x update. Same per-element arithmetic as above.
void launch_cg_update_p_ring(size_t n, const CgScalars* s, const double* r, const double* p_in, double* p_out,
                             int iteration, hipStream_t stream, bool reverse = false, bool fma_form = false);
// x = x_in + sum_j alpha[slot_j] * p[slot_j], slot_j = (first_slot + j) % slots for j = 0..count-1, added in that
// order with one fma each: element for element the x the per-iteration updates x += alpha_j p_j produce.
constexpr int kMaxRingSlots = 16;
struct RingSlots {
    const double* p[kMaxRingSlots];
};
// s (may be null) / window_start: only terms of iterations window_start + 1 ... s->iterations are added (a host that ran one
// iteration ahead may ask for one term too many: that iteration was never counted and its alpha slot holds an old value).
// x_in == nullptr: x_in is known to hold +0.0 everywhere and is not loaded; the chain starts from 0.0, same bits.
void launch_cg_flush_x(size_t n, const double* alphas, const RingSlots& ring, int slots, int first_slot, int count,
                       const double* x_in, double* x, hipStream_t stream, const CgScalars* s = nullptr, int window_start = 0);
int cg_partial_count(size_t n);  // partial slots written by the two reducing kernels above
// *d_out = sum of partials[0..count) and extra[0..extra_count) in a fixed order (reduce_device.hpp: slices of `partials`, then
// [slice sums | extra]), in ONE launch. extra: the partials of a split SpMV's boundary rows (may be null).
// host_progress (may be null): int in host-coherent pinned memory, set to progress_value once the sum is stored;
// read by the solver's watchdog report.
// mailbox (may be null; comm.hpp): the sum is completed across the ranks inside the same launch.
void launch_reduce_partials(const double* partials, int count, double* d_out,
                            const int* d_skip_flag, hipStream_t stream, const ReduceScratch& scratch = ReduceScratch{},
                            int* host_progress = nullptr, int progress_value = 0,
                            const PeerMailbox* mailbox = nullptr, const double* extra = nullptr, int extra_count = 0);
// The rows a slab's neighbours wait for: [0, count_a) and [second, second + count_b), all even (its first / last grid row,
// rounded outwards to 4 KiB).
struct EdgeRows {
    size_t count_a, second, count_b;
};
// The same reduction followed by launch_cg_scalars_step() in the same launch
// (only valid when no all-reduce has to happen between the sum and the step).
void launch_reduce_partials_and_step(const double* partials, int count, double* d_out, const int* d_skip_flag,
                                     hipStream_t stream, const ReduceScratch& scratch, CgScalars* s, double tol, double* history,
                                     int* host_record, int sequence, double* alpha_ring = nullptr, int ring_slots = 0,
                                     const PeerMailbox* mailbox = nullptr, int* host_progress = nullptr,
                                     int progress_value = 0);
// The scalar step (optional: step_host_record == nullptr means an earlier launch took it), the direction update p_out = r + beta p_in
// of the EdgeRows (optional) and of rows [bulk_lo, bulk_lo + bulk_rows) in ONE launch (round 5): no workgroup waits for the
// step -- each derives beta and the convergence verdict from the scalars the step does not touch (CgScalars::rr_ring) with
// the step's own expressions. The first workgroups take the edge rows, write them through and raise the scratch's edges_ready
// to `sequence` (the side stream's exchange is released by that flag, launch_edges_wait), the rest streams the bulk.
// iteration: as launch_cg_update_p_ring's. All row counts even. One launch instead of three on the RCCL path (step | edge rows |
// rest), instead of two elsewhere; no event between them.
struct DirectionLaunch {
    CgScalars* s;
    double tol;
    int iteration;
    double* history;       // the step's (may be null)
    int* step_host_record; // null: no step in this launch
    int sequence;
    double* alpha_ring;
    int ring_slots;
    const double* r;
    const double* p_in;
    double* p_out;
    size_t bulk_lo, bulk_rows;
    bool reverse, fma_form;
};
void launch_cg_direction(const DirectionLaunch& d, const EdgeRows* edge_rows, const ReduceScratch& scratch, hipStream_t stream);
// Side stream: one thread waits (bounded) until the step-and-edges launch `sequence` on the compute stream has written its edge
// rows through to memory; the halo exchange enqueued behind it then needs no cross-stream event. *late = 3 if it gave up.
void launch_edges_wait(const ReduceScratch& scratch, int sequence, long long timeout_ticks, int* late, hipStream_t stream);
// After the (all-reduced) r.r is known: b_norm (first call), residual, history, convergence
// flag, beta, rr_old <- rr_new, iteration counter.
void launch_cg_scalars_init(CgScalars* s, double* history, hipStream_t stream);
// host_record (may be null): three ints in host-coherent pinned memory, {sequence, converged, iterations};
// the kernel publishes the iteration's status there so the host needs no copy command on the stream.
// alpha_ring (may be null): alpha of the iteration is also stored at alpha_ring[(iterations - 1) % ring_slots].
void launch_cg_scalars_step(CgScalars* s, double tol, double* history, int* host_record, int sequence,
                            hipStream_t stream, double* alpha_ring = nullptr, int ring_slots = 0);

}  // namespace spmv_amd
