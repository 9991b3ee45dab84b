/* spmv_amd/api.h -- entry points of libspmv_amd.so.
 *
 * Part 1 re-declares, under the reference's own names and signatures, every
 * function the reference's harness calls on the SpMV + CG path, so that the
 * harness objects link against this library instead of the reference's
 * src/spmv, src/solvers and src/io objects. Each declaration cites the reference
 * declaration it replaces. Linkage (C vs C++) follows the reference header.
 *
 * Part 2 is the FFI surface: the same operations as plain `extern "C"`
 * functions taking only pointers, ints and doubles (structs by pointer), plus
 * the few things a caller without a HIP binding needs (device buffers, on-stream
 * timing, the multi-GPU communicator hook and a resident CG state so that a
 * benchmark can time solves with everything already in HBM).
 */
#ifndef SPMV_AMD_API_H
#define SPMV_AMD_API_H

#include <stddef.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif
#include "spmv_amd/types.h"

/* ===================================================================== *
 * Part 1 -- reference-named boundary                                     *
 * ===================================================================== */

#ifdef __cplusplus
extern "C" {
#endif

/* Process-wide host matrices. Populated by build_csr_struct / the operators'
 * init, read by calculate_spmv_metrics and by cg_solve_mgpu_partitioned.
 * reference: include/spmv.h:34,39 ; src/spmv/spmv_cusparse_csr.cu:23 */
extern CSRMatrix csr_mat;
extern ELLPACKMatrix ellpack_matrix;

/* reference: include/spmv.h:37-38 (declared there, defined nowhere in src/) */
int build_ellpack_from_csr_local(CSRMatrix* csr_matrix);
int ensure_ellpack_structure_built(MatrixData* mat);

/* Operator lookup. Canonical names: "stencil5-csr", "cusparse-csr", "stencil7-csr", "ellpack",
 * "stencil5-ellpack"; accepted aliases: "stencil5", "csr", "stencil7". Unknown -> NULL.
 * reference: include/spmv.h:141-150 ; src/spmv/spmv.cu:11-23 */
SpmvOperator* get_operator(const char* mode);

/* reference: include/spmv.h:159-183 ; src/spmv/spmv_metrics.cu:46-102,190-324 ;
 * src/spmv/gpu_detection.cu */
void calculate_spmv_metrics(double execution_time_ms, const MatrixData* mat,
                            const char* operator_name, BenchmarkMetrics* metrics);
int get_gpu_properties(BenchmarkMetrics* metrics);
void print_benchmark_metrics(const BenchmarkMetrics* metrics, FILE* output_file);
void print_metrics_json(const BenchmarkMetrics* metrics, FILE* output_file);
void print_metrics_csv(const BenchmarkMetrics* metrics, FILE* output_file);

/* Matrix Market I/O. reference: include/io.h:71-134 ; src/io/io.cu */
int read_matrix_type(const char* filename);
void read_matrix_general(MatrixData* mat, const char* filename, int* rows, int* cols, int* nnz,
                         int** csr_rowptr, int** csr_colind, double** csr_val);
void read_matrix_symtogen(MatrixData* mat, const char* filename, int* rows, int* cols, int* nnz,
                          int** csr_rowptr, int** csr_colind, double** csr_val, int* nnz_general);
int load_matrix_market(const char* filename, MatrixData* mat);
void convert_csr_to_ellpack(const struct CSRMatrix* csr_matrix,
                            struct ELLPACKMatrix* ellpack_matrix, int* max_width);
int write_matrix_market_stencil5(int n, const char* filename);
/* The n x n x n 7-point stencil, point (k, i, j) = row k n^2 + i n + j, neighbours at -+1 (W/E), -+n (N/S), -+n^2 (D/U): centre 7.0,
 * every neighbour -1.0 (strictly diagonally dominant, SPD; sum(A 1) = n^3 + 6 n^2); write_matrix_market_stencil5's format with the
 * same "% STENCIL_GRID_SIZE n" comment, entry order C, W, E, N, S, D, U per point; 7 n^3 - 6 n^2 entries. 1 <= n <= 674, else 1. */
int write_matrix_market_stencil7(int n, const char* filename);

/* N-run statistics with >2 sigma outlier removal and median.
 * reference: include/benchmark_stats.h:23-29 ; include/benchmark_stats_mgpu.h:12-15 ;
 * src/spmv/benchmark_stats.cu ; src/spmv/benchmark_stats_mgpu_partitioned.cu */
int benchmark_with_stats(int (*run_func)(const double*, double*, double*), const double* x,
                         double* y, int num_runs, BenchmarkStats* stats);
int cg_benchmark_with_stats_device(SpmvOperator* spmv_op, MatrixData* mat, double* b, double* x,
                                   CGConfig config, int num_runs, BenchmarkStats* bench_stats,
                                   CGStats* final_stats);
int cg_benchmark_with_stats_mgpu_partitioned(SpmvOperator* spmv_op, MatrixData* mat, double* b,
                                             double* x, CGConfigMultiGPU config, int num_runs,
                                             BenchmarkStats* bench_stats,
                                             CGStatsMultiGPU* final_stats);

/* reference: include/solvers/cg_metrics.h:23-37 ; src/solvers/cg_metrics.cu */
void export_cg_json(const char* filename, const char* mode, const MatrixData* mat,
                    const BenchmarkStats* bench_stats, const CGStats* cg_stats);
void export_cg_mgpu_json(const char* filename, const char* mode, const MatrixData* mat,
                         const BenchmarkStats* bench_stats, const CGStatsMultiGPU* cg_stats,
                         int num_gpus);
void export_cg_csv(const char* filename, const char* mode, const MatrixData* mat,
                   const BenchmarkStats* bench_stats, const CGStats* cg_stats, bool write_header);

#ifdef __cplusplus
} /* extern "C" */
#endif

#ifdef __cplusplus
/* C++ linkage, as in the reference headers. */

/* reference: include/spmv.h:137-139 */
extern SpmvOperator SPMV_CSR;               /* "cusparse-csr": own CSR kernels, no vendor library */
extern SpmvOperator SPMV_STENCIL5_CSR;      /* "stencil5-csr" */
extern SpmvOperator SPMV_STENCIL7_CSR;      /* "stencil7-csr" (new: the n x n x n 7-point stencil, see spmv_amd_init_stencil7_synthetic) */
extern SpmvOperator SPMV_STENCIL_HALO_MGPU; /* "stencil5-halo-mgpu": declared, never defined upstream */
extern SpmvOperator SPMV_ELLPACK;           /* "ellpack" (new: upstream ships headers only) */
extern SpmvOperator SPMV_STENCIL5_ELLPACK;  /* "stencil5-ellpack": ELL values, computed columns */

/* COO -> CSR with per-row insertion sort by column; fills csr_mat.
 * reference: include/spmv_csr.h:47 ; src/spmv/spmv_cusparse_csr.cu:62-170 */
int build_csr_struct(struct MatrixData* mat);

/* reference: include/spmv_ellpack.h:50-51 (declaration only upstream) */
int build_ellpack_from_csr_struct(const struct CSRMatrix* csr_matrix, ELLPACKMatrix* ellpack_matrix,
                                  int* max_width);

/* reference: include/solvers/cg_solver.h:59-77 ; src/solvers/cg_solver.cu:154-378,436-706 */
int cg_solve(SpmvOperator* spmv_op, MatrixData* mat, const double* b, double* x, CGConfig config,
             CGStats* stats);
int cg_solve_device(SpmvOperator* spmv_op, MatrixData* mat, const double* b, double* x,
                    CGConfig config, CGStats* stats);

/* 1-D row-slab CG over all ranks of the world communicator (see
 * spmv_amd_comm_set_world; none set = one rank). spmv_op is unused, callers pass
 * NULL. b and x are full-length host arrays on every rank; on return rank 0's x
 * holds the gathered solution.
 * reference: include/solvers/cg_solver_mgpu_partitioned.h:50-51 ;
 * src/solvers/cg_solver_mgpu_partitioned.cu:236-908 */
int cg_solve_mgpu_partitioned(SpmvOperator* spmv_op, MatrixData* mat, const double* b, double* x,
                              CGConfigMultiGPU config, CGStatsMultiGPU* stats);
#endif /* __cplusplus */

/* ===================================================================== *
 * Part 2 -- FFI surface (all extern "C", prefix spmv_amd_)               *
 * ===================================================================== */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FFI aliases of the C++-linkage entry points above (configs by pointer) ---- */
int spmv_amd_build_csr_struct(MatrixData* mat);
int spmv_amd_build_ellpack_from_csr_struct(const CSRMatrix* csr, ELLPACKMatrix* ell,
                                           int* max_width);
int spmv_amd_cg_solve(SpmvOperator* op, MatrixData* mat, const double* b, double* x,
                      const CGConfig* config, CGStats* stats);
int spmv_amd_cg_solve_device(SpmvOperator* op, MatrixData* mat, const double* b, double* x,
                             const CGConfig* config, CGStats* stats);
int spmv_amd_cg_solve_mgpu_partitioned(MatrixData* mat, const double* b, double* x,
                                       const CGConfigMultiGPU* config, CGStatsMultiGPU* stats);

/* Drops the host CSR/ELL held in csr_mat / ellpack_matrix (the reference keeps
 * them for the life of the process; tests that load several matrices need this). */
void spmv_amd_reset_host_matrices(void);

/* ---- integer helpers that must match the reference bit for bit ---- */

/* CSR start of interior row `row` of an n x n 5-point stencil.
 * reference: calculate_interior_csr_offset, src/spmv/spmv_stencil_csr_direct.cu:50-67 */
int spmv_amd_interior_csr_offset(int row, int grid_size);

/* CSR start of row `row` (= k n^2 + i n + j) of the n x n x n 7-point stencil whose rows are sorted by column ([D,N,W,C,E,S,U]
 * minus the absent ones), in closed form; row == n^3 gives the total, 7 n^3 - 6 n^2. -1 for n < 1, n > 2^20 (the arithmetic is 64-bit) or a row outside [0, n^3]. */
long long spmv_amd_stencil7_row_start(long long row, int n);

/* Row slab of `rank`: n / world rows each, the last rank takes the remainder.
 * reference: src/solvers/cg_solver_mgpu_partitioned.cu:261-268 */
void spmv_amd_partition_rows(int n, int world, int rank, int* row_offset, int* n_local);

/* ---- device plumbing for callers that have no HIP binding of their own ---- */
int spmv_amd_device_count(void);
int spmv_amd_set_device(int device);
/* The calling thread's current device; pci_bus_id (may be NULL) receives "0000:c1:00.0"-style text. */
int spmv_amd_current_device(char* pci_bus_id, int cap);
void* spmv_amd_device_alloc(size_t bytes);
void spmv_amd_device_free(void* d_ptr);
int spmv_amd_copy_to_device(void* d_dst, const void* h_src, size_t bytes);
int spmv_amd_copy_to_host(void* h_dst, const void* d_src, size_t bytes);
int spmv_amd_device_fill_f64(double* d_ptr, size_t count, double value);
int spmv_amd_device_synchronize(void);

/* Measurement aid: the rate this GPU sustains for the byte mix of one STENCIL5 row (48 B read : 8 B written,
 * SURVEY.md 8d) with ideal accesses -- coalesced 8-byte nontemporal loads / stores, no neighbours, no row
 * structure -- on the benchmark's own data. `warmup` untimed launches over `rows` rows, then `reps` launches
 * timed one by one with HIP events on the launch stream (ms_each[reps]). Returns bytes moved per launch. */
double spmv_amd_stream_ceiling(size_t rows, int warmup, int reps, float* ms_each);
/* The same probe for the byte mix of another format at five entries per row: mix 0 = STENCIL5 (56 B/row, as above),
 * 1 = CSR (80 B/row: values, column indices, row pointers, x, y), 2 = ELLPACK width 5 (76 B/row). The index
 * streams are read, nothing is gathered through them: what the streams alone cost on this GPU. */
double spmv_amd_stream_ceiling_mix(int mix, size_t rows, int warmup, int reps, float* ms_each);

/* ---- operators on synthetic, device-generated matrices ---- */

/* Initialises operator `mode` on the n x n 5-point stencil of
 * write_matrix_market_stencil5 (centre 5.0, neighbours -1.0) with the CSR/ELL
 * arrays produced directly in HBM by a generator kernel: same bytes as
 * load_matrix_market + init would upload, without the host COO/CSR (58 GB at
 * n = 20000). csr_mat gets the dimensions, its host arrays stay NULL. */
int spmv_amd_init_stencil5_synthetic(const char* mode, int n);

/* The same for the n x n x n 7-point stencil of write_matrix_market_stencil7 (centre 7.0, neighbours -1.0): `mode` is
 * "stencil7-csr" or "cusparse-csr" (the ELLPACK operators return failure). Rows (n^3) and entries (7 n^3 - 6 n^2) must fit int32:
 * n < 1 and n > 674 are refused with a message before any HIP call.
 * "stencil7-csr" contract: a matrix is the operator's own when MatrixData.grid_size = n >= 2, rows == cols == n^3 and every row has the
 * complete pattern [D,N,W,C,E,S,U] (checked on the device at init); variants "stencil7/row-lds" (n >= SPMV_AMD_STENCIL7_ROWLDS_MIN_GRID,
 * default 64) and "stencil7/row-direct"; anything else initialises and runs the CSR kernels as "stencil7/csr-loop". Every row, in
 * every variant, is sum = 0.0 ; sum = fma(v[k], x[col[k]], sum) for ascending k ; y = sum: bit for bit the sequential CSR sum. */
int spmv_amd_init_stencil7_synthetic(const char* mode, int n);
/* The same with the centre and the neighbours' coefficient chosen by the caller (6.0 / -1.0: the Poisson matrix with Dirichlet
 * boundaries): spmv_amd_init_stencil7_synthetic(mode, n) is this with 7.0 / -1.0. */
int spmv_amd_init_stencil7_synthetic_values(const char* mode, int n, double center, double off);

/* y = alpha*A*x + beta*y on an initialised "ellpack" / "stencil5-ellpack" operator: the full
 * contract of the kernel prototyped in reference include/spmv_stencil.h:25-42 (the operator table
 * itself always runs alpha = 1, beta = 0). Device pointers, default stream, no synchronisation. */
int spmv_amd_ellpack_run_device_scaled(const char* mode, const double* d_x, double* d_y, double alpha,
                                       double beta);

/* Downloads the device CSR of an initialised CSR-based operator (tests compare
 * it with build_csr_struct's host result). Any pointer may be NULL. */
int spmv_amd_download_device_csr(const char* mode, int* row_ptr, int* col_idx, double* values);

/* Launches run_device `reps` times back to back on the operator's stream and
 * returns each launch's duration from HIP events recorded on that stream.
 * d_x / d_y == NULL: the operator's own staging vectors, i.e. what run_timed's kernel reads and writes
 * (x set to 1.0, the reference benchmark's input; y placed by the operator at init, see below). */
int spmv_amd_time_run_device(const char* mode, const double* d_x, double* d_y, int reps,
                             float* ms_each);
/* Output placement. On MI355X a SpMV runs ~4.5 % faster when the vector it WRITES lies in another class of 32 GiB
 * address regions than the data it reads (csrc/device_runtime.hpp; profiles/r04_spmv_regions.txt), and only hipMalloc
 * decides the class: at init every operator times its kernel on up to SPMV_AMD_PLACEMENT_CANDIDATES (default 3, one region apart; 1 = off)
 * allocations for its y vector and keeps the fastest (vectors of >= 16 Mi rows). Reports how many were timed and
 * kernel time on the first / on the one kept. Returns 0 for an unknown or uninitialised operator. */
int spmv_amd_operator_placement(const char* mode, int* candidates, double* gain);

/* Which kernel variant the last init selected: a static string, one of
 * "stencil5/row-lds" (default on verified stencils with grid >= 512), "stencil5/row-direct"
 * (default on smaller verified stencils), "stencil5/row-generic", "stencil5/row-generic(csr-loop)";
 * "csr/stream", "csr/adaptive", "csr/row-scalar", "csr/wavefront"; "ell/slot-major", "ell/stencil5-direct". */
const char* spmv_amd_operator_variant(const char* mode);

/* Forces a kernel variant of `mode` ("row-lds", "row-direct", "row-generic" / "stream", "adaptive", "row-scalar",
 * "wavefront"; NULL or "auto" = automatic). A variant
 * whose preconditions the matrix does not meet falls back to the next applicable one. */
int spmv_amd_operator_select_variant(const char* mode, const char* variant);

/* ---- the CG building blocks one at a time (device pointers, each call synchronises) ----
 * reference kernels: axpy_kernel / axpby_kernel (cg_solver.cu:38-54), axpy_kernel_device /
 * axpy_sub_kernel_device (:59-74), update_p_kernel (:90-95), dot_kernel + final_sum_kernel (:110-132,384-409). */
int spmv_amd_blas1_axpy(size_t n, double a, const double* d_x, double* d_y);
int spmv_amd_blas1_axpby(size_t n, double a, const double* d_x, double b, const double* d_y, double* d_z);
int spmv_amd_blas1_axpy_dev(size_t n, double a, const double* d_x, double* d_y, int subtract);
int spmv_amd_blas1_update_p_dev(size_t n, const double* d_r, double b, double* d_p);
int spmv_amd_blas1_dot(size_t n, const double* d_x, const double* d_y, double* result);
/* The slab solver's fused steps on caller data. which = 0: r -= (rr_old/pAp)*Ap and r.r (d_a = Ap, d_b = r);
 * 1: p_out = r + beta*p_in (d_a = r, d_b = p_in, d_c = p_out); 2: r = b - Ap, p = r and r.r (d_a = b, d_b = Ap,
 * d_c = [r | p], 2n doubles). scalars = {rr_old, pAp, beta}. reverse: sweep direction (results must not depend on it). */
int spmv_amd_cg_fused_step(int which, size_t n, const double* scalars, const double* d_a, double* d_b, double* d_c,
                           int reverse, double* dot_out);

/* ---- residual history of the most recent CG solve in this process ---- */
/* Copies ||r_k||, k = 0..iterations, into out (at most cap values); returns how
 * many the solve recorded. */
int spmv_amd_cg_last_history(double* out, int cap);
/* cg_solve_device keeps its five vectors and direction ring between calls (the harness solves one system 13 times,
 * reference src/main/cg_solver.cu:154-178). They are released by the free() of any of this library's operators, or here --
 * the call for a caller that drives its own SpmvOperator table through cg_solve_device. Safe to call at any time.
 * The batched solver's workspace (spmv_amd_cg_solve_device_multi) is released together with this one. */
void spmv_amd_cg_release_workspace(void);

/* ---- several right-hand sides per matrix pass (csrc/spmm_kernels.hip, csrc/cg_multi.hip) ----
 * Block vectors on the device are ROW-INTERLEAVED: element (row, column j) of a block of nrhs columns is X[row * nrhs + j]
 * (one lane reads a row's nrhs values as one run; the solver streams 4-5 arrays instead of 4-5 nrhs). On the host they are
 * nrhs vectors one after the other (numpy (nrhs, n) in C order); the two helpers below convert. nrhs is 1 to 8.
 * "stencil5-csr" and "cusparse-csr" have the multi-RHS path ("ellpack" / "stencil5-ellpack" and caller-supplied operator
 * tables do not). Column j of every result is computed by exactly the arithmetic of the single-vector path on column j
 * (csrc/stencil_row_device.hpp): it depends on column j's data only, not on nrhs nor on the other columns.
 * Every entry point checks its arguments (nrhs outside 1..8, null pointers, an operator without the path or not initialised)
 * before any HIP call and returns non-zero with a message on stderr. */

/* Y = A X on an initialised operator, X of `cols` rows, Y of `rows` rows (device pointers, 8-byte aligned; 16-byte aligned
 * with an even nrhs take 16-byte loads). Default stream, no synchronisation. The coefficients are read once for all columns;
 * the kernel follows the operator's single-vector variant (spmv_amd_operator_select_variant). */
int spmv_amd_spmm_device(const char* mode, int nrhs, const double* d_X, double* d_Y);
/* Which SpMM kernel the operator's multi-RHS path takes (a static string): "spmm/stencil5-row-lds", "spmm/stencil5-row-direct",
 * "spmm/stencil5-row-generic", "spmm/stencil5-row-generic(csr-loop)", "spmm/csr"; "none", "uninitialised", "unknown-operator". */
const char* spmv_amd_spmm_variant(const char* mode);
/* host (nrhs, n) columns <-> device interleaved block of n rows (synchronous; a temporary device copy of the block). */
int spmv_amd_block_to_device(int nrhs, size_t n, const double* host_columns, double* d_X);
int spmv_amd_block_to_host(int nrhs, size_t n, const double* d_X, double* host_columns);
/* nrhs INDEPENDENT CG solves on one operator (not block CG): each column has its own alpha, beta, stopping test, history and
 * iteration count, with cg_solve_device's stopping rule, statistics and verbose semantics; a converged column is frozen
 * while the others go on. Only the SpMM is shared. B, X: host, nrhs vectors of length mat->rows one after the other; X in =
 * x0, out = solution. stats: nrhs entries; time_total_ms is the wall time of the whole batch (the same in every column), the
 * breakdown is filled with enable_detailed_timers only; the upload of B / x0 and the download of X are outside the timed
 * region. The workspace (four block vectors) is sized against the device's free memory first: a batch that does not fit is
 * refused with a message and a non-zero return. It is kept between calls and released with cg_solve_device's (an
 * operator's free(), spmv_amd_cg_release_workspace()). */
int spmv_amd_cg_solve_device_multi(SpmvOperator* op, MatrixData* mat, int nrhs, const double* B, double* X,
                                   const CGConfig* config, CGStats* stats);
/* Residual history of column `rhs` of the last batched solve, like spmv_amd_cg_last_history; -1 if there is no such column. */
int spmv_amd_cg_last_history_multi(int rhs, double* out, int cap);
/* Device bytes the batched solver's workspace holds now: 0 once it is released (operator free(),
 * spmv_amd_cg_release_workspace()) or before the first batched solve. No HIP call. */
size_t spmv_amd_cg_multi_workspace_bytes(void);

/* ---- preconditioned CG (csrc/pcg.hip, the preconditioner record csrc/precond.hip) ----
 * z = M^-1 r with M = diag(A) ("jacobi") or I ("none"); otherwise the algebra, stopping rule (true residual, strict <, the
 * converging iteration counted), statistics, timer rule and verbose semantics of cg_solve_device (verbose lines tagged
 * [PCG-DEVICE]). A pAp or r.z that is zero or not finite stops the solve in that iteration with converged = 0 and x finite;
 * there is no sign test, so negative-definite systems solve. Results are deterministic: the same solve twice gives bit-identical
 * x and history. Every entry point checks its arguments before any HIP call and returns NULL / non-zero with a message on
 * stderr. */
typedef struct SpmvAmdPrecond SpmvAmdPrecond;
/* A preconditioner for an initialised, square operator of this library ("stencil5-csr", "cusparse-csr", "ellpack",
 * "stencil5-ellpack"). kind "none" | "jacobi". Jacobi reads the operator's own device storage: d_i = the sum of row i's
 * entries in column i (CSR order, from 0.0), dinv_i = 1.0 / d_i -- the same bits from every operator for the same matrix.
 * Every d_i must be finite, non-zero and of d_0's sign. NULL on refusal; *bad_row (may be NULL) = the first offending row,
 * or -1 when the refusal is not about a row. The preconditioner belongs to the operator's current matrix: after the operator's
 * free() or next init it is refused by spmv_amd_pcg_solve_device. */
SpmvAmdPrecond* spmv_amd_precond_create(SpmvOperator* op, const char* kind, int* bad_row);
/* Jacobi from a caller's device diagonal of n values (the same validity rule): the way in for operators this library does
 * not own. Usable with any operator of n rows. */
SpmvAmdPrecond* spmv_amd_precond_create_from_diagonal(const double* d_diag, int n, int* bad_row);
/* Kind "chebyshev" (DESIGN.md section 14): z = M^-1 r is the degree-`degree` Chebyshev polynomial in B = D^-1 A on [lambda_min,
 * lambda_max], applied with SpMVs and streaming updates only; degree 0 is Jacobi scaled by c0. The operator must be one of this
 * library's (there is no from-diagonal form); dinv = 1 / d under Jacobi's validity rule (*bad_row as there). degree: 0..32 = steps =
 * SpMVs per application. lambda_max > 0: used as given; otherwise the symmetric Gershgorin bound max_i sum_j |a_ij| sqrt(|dinv_i|
 * |dinv_j|), row i summed in storage order from 0.0 (a bound on D^-1/2 A D^-1/2, invariant under symmetric diagonal scaling).
 * lambda_min > 0: used as given; otherwise lambda_max / 30.0. Refused (NULL) unless 0 < lambda_min < lambda_max, both finite; a NaN or
 * infinite argument, a degree out of range, a null or uninitialised operator are refused before any HIP call.
 * Coefficients, host fp64, one rounding per operation, in this order: theta = 0.5 (lmax + lmin); delta = 0.5 (lmax - lmin);
 * sigma = theta / delta; c0 = 1.0 / theta; rho = 1.0 / sigma; for k = 1..degree: rho' = 1.0 / (2.0 sigma - rho); h_k = rho' rho;
 * g_k = 2.0 rho' / delta; rho = rho'.
 * Application, element-wise:  term 0: u = dinv r; d = c0 u; z = d.   step k: w = A z (the operator's own bits); t = fma(-1.0, w, r);
 * u = dinv t; d = fma(g_k, u, h_k d); z = z + d.
 * With lambda_max a true upper bound M^-1 A has its spectrum in (0, 2): PCG stays valid; negative-definite matrices work as under
 * Jacobi. On a well-conditioned matrix the polynomial costs more than it saves (DESIGN.md section 14 has the numbers). */
SpmvAmdPrecond* spmv_amd_precond_create_chebyshev(SpmvOperator* op, int degree, double lambda_min, double lambda_max, int* bad_row);
/* degree, interval, and up to cap coefficients in the order c0, h_1, g_1, h_2, g_2, ...; returns how many exist (1 + 2*degree);
 * 0 for another kind (nothing is written). Any out pointer may be NULL. */
int spmv_amd_precond_chebyshev_info(const SpmvAmdPrecond* m, int* degree, double* lambda_min, double* lambda_max, double* coefficients, int cap);
/* Kind "multigrid" (csrc/multigrid.hip), for "stencil5-csr" on a verified complete 5-point stencil: z = M^-1 r is one
 * symmetric V(nu, nu) cycle, nu = smoother_degree (0..8), on a hierarchy of 5-point stencils made by 2 x 2 aggregation. max_levels: 0 =
 * automatic, else 1..32 caps the number of levels. Refused before any HIP call: a null operator, an argument out of range, an operator
 * that is not stencil5-csr or not initialised; after HIP work: a matrix that is not a verified stencil, a diagonal entry on any level
 * that breaks Jacobi's validity rule (the level is named on stderr, *bad_row = the row of that level). spmv_amd_precond_create(op,
 * "multigrid") stays refused: this kind has arguments.
 * Levels: level 0 is the operator's n0 x n0 grid; level l+1 has the grid ceil(n_l / 2); aggregate (I, J) = the fine points (2I + a, 2J + b),
 * a, b in {0, 1}, that exist. Coarsening stops at the first level with n_l <= 8, or at max_levels.
 * Coarse operator A_c = P^T A P, P piecewise constant, again a complete 5-point CSR ([N,W,C,E,S]); every entry a sequential sum from
 * 0.0 with plain additions: the members in the order (0,0), (0,1), (1,0), (1,1), each member's entries in CSR order, every entry added
 * to the coarse entry of the aggregate its column lies in (N_c = sum_b N(2I, 2J+b), W_c = sum_a W(2I+a, 2J), E_c = sum_a E(2I+a, 2J+1),
 * S_c = sum_b S(2I+1, 2J+b), C_c = everything that stays inside). A bit-symmetric fine matrix gives a bit-symmetric coarse one.
 * Per level: dinv by the diagonal pass above, lambda_max by the symmetric Gershgorin bound; the smoother is the Chebyshev application of
 * degree nu on [lambda_max / 4.0, lambda_max]; the coarsest level is solved by degree 8 on [lambda_max / 30.0, lambda_max] from a
 * zero guess (term 0 and eight steps).
 * Cycle on level l, input r, output z:  (1) term 0, then steps 1..nu.  (2) r_c[I,J] = ((t00 + t01) + t10) + t11 over the members that
 * exist, t_i = fma(-1.0, (A z)_i, r_i), (A z)_i the bits of stencil5-csr's SpMV for row i.  (3) e_c = cycle(l+1, r_c).
 * (4) z = fma(2.0, e_c[agg(i)], z).  (5) nu + 1 updates t = fma(-1.0, (A z), r); u = dinv t; d = fma(g, u, h d); z = z + d: the first with
 * g = c0, h = 0.0 and d as step (1) left it, then steps 1..nu with (h_k, g_k).
 * csrc/mg_schedule.hpp states this order once; the single-vector and the batched cycle (..._multigrid_multi below) both walk it.
 * The solve with this kind reads the iteration's verdict on the host before the cycle: the converging iteration runs none. */
SpmvAmdPrecond* spmv_amd_precond_create_multigrid(SpmvOperator* op, int smoother_degree, int max_levels, int* bad_row);
/* Kind "multigrid" for "stencil7-csr" (csrc/multigrid3d.hip): the cycle above on a hierarchy of 7-point stencils made
 * by 2 x 2 x 2 aggregation of the operator's n^3 grid. The operator must run a verified complete 7-point stencil (n >= 2): any other
 * operator ("stencil5-csr" included) and a "stencil7/csr-loop" plan (a matrix that is not the complete pattern, or the forced variant)
 * are refused, like a null operator, a smoother_degree outside 0..8 and a max_levels outside 0..32, before any HIP call with
 * *bad_row = -1; a diagonal entry on any level that breaks Jacobi's validity rule is refused after HIP work (the level is named on
 * stderr, *bad_row = the row of that level). A refusal leaves no device memory behind. spmv_amd_precond_create_multigrid keeps
 * refusing "stencil7-csr".
 * Levels: level 0 is the operator's grid n_0; n_{l+1} = ceil(n_l / 2); aggregate (K, I, J) = the fine points (2K + c, 2I + a, 2J + b),
 * c, a, b in {0, 1}, that exist (point (k, i, j) = row k n^2 + i n + j). Coarsening stops at the first level with n_l <= 8, or at max_levels.
 * Coarse operator A_c = P^T A P, P piecewise constant, again a complete 7-point CSR ([D,N,W,C,E,S,U] = columns -n^2, -n, -1, 0, +1, +n,
 * +n^2); every entry a sequential sum from 0.0 with plain additions: the members in the order (c, a, b) = (0,0,0), (0,0,1), (0,1,0),
 * (0,1,1), (1,0,0), (1,0,1), (1,1,0), (1,1,1), each member's entries in CSR order, every entry added to the coarse entry of the
 * aggregate its column lies in (D_c = the D entries of the four members with c = 0, in member order; U_c those of c = 1; N_c / S_c
 * the N / S entries of a = 0 / a = 1; W_c / E_c the W / E entries of b = 0 / b = 1; C_c everything that stays inside, twenty-four
 * terms in a full aggregate). A bit-symmetric fine matrix gives a bit-symmetric coarse one.
 * Per level: as above -- dinv by the diagonal pass, lambda_max by the symmetric Gershgorin bound, the smoother of degree nu on
 * [lambda_max / 4.0, lambda_max], the coarsest level by degree 8 on [lambda_max / 30.0, lambda_max] from a zero guess.
 * Cycle: steps (1) to (5) above with  (2) r_c[K,I,J] = (((((((t000 + t001) + t010) + t011) + t100) + t101) + t110) + t111) over the
 * members t_cab that exist, t_i = fma(-1.0, (A z)_i, r_i), (A z)_i the bits of stencil7-csr's SpMV for row i: for EVERY row, interior or
 * not, sum = 0.0 ; sum = fma(v[k], z[col[k]], sum) for ascending k;  (4) z = fma(2.0, e_c[agg(i)], z): the factor stays 2.0, the Galerkin
 * face coupling of 2 x 2 x 2 aggregates being twice the re-discretised one as in 2-D. */
SpmvAmdPrecond* spmv_amd_precond_create_multigrid3d(SpmvOperator* op, int smoother_degree, int max_levels, int* bad_row);
/* The number of levels, nu, and up to cap grids n_l (the edge of the n_l x n_l or n_l x n_l x n_l grid) and lambda_max_l; returns the
 * number of levels, 0 for another kind (nothing is written). Any out pointer may be NULL. */
int spmv_amd_precond_multigrid_info(const SpmvAmdPrecond* m, int* levels, int* smoother_degree, int* grids, double* lambda_max, int cap);
/* 2 for a multigrid preconditioner of stencil5-csr, 3 for one of stencil7-csr, 0 for NULL, any other kind and a handle of
 * spmv_amd_precond_create_amg (there is no grid). */
int spmv_amd_precond_multigrid_dimension(const SpmvAmdPrecond* m);
/* Kind "multigrid" for "cusparse-csr", the general CSR operator (csrc/amg.hip, csrc/amg_setup.hpp): the cycle of
 * spmv_amd_precond_create_multigrid on a hierarchy made by aggregating the MATRIX -- a 9-point stencil, a rectangular grid, a matrix
 * read from a file, a permuted stencil, a graph Laplacian. nu = smoother_degree (0..8); max_levels: 0 = automatic (32), else 1..32;
 * strength = theta, finite and in [0, 1) (the application uses 0.08). Refused before any HIP call, *bad_row = -1: a null operator, an
 * argument out of range, an operator that is not cusparse-csr (named in the sentence; stencil5-csr and stencil7-csr have creators of
 * their own and their product bits follow another order: to compare, load the same matrix into cusparse-csr), one used before init, a
 * matrix that is not square. Refused after HIP work: a diagonal entry on any level that breaks Jacobi's validity rule (the level is
 * named on stderr, *bad_row = the row of that level). The set-up runs on the host from the operator's CSR read back; everything is
 * sized against the device's free memory before anything is allocated; a refusal leaves no device memory behind.
 * The handle is a "multigrid" handle: spmv_amd_pcg_solve_device, spmv_amd_gcr_solve_device and spmv_amd_precond_apply_device accept it;
 * spmv_amd_bicgstab_solve_device and every batched entry point refuse it with the sentences they have (its hierarchy holds single
 * vectors); spmv_amd_precond_multigrid_info works on it and writes 0 into every grids entry.
 * All host arithmetic is fp64 with one rounding per operation.
 * Diagonal: d_i and dinv_i of a level by the diagonal pass above, with its validity rule.
 * Strong couplings: t2 = theta theta; entry k of row i with column j != i and value v is strong iff v v > t2 fabs(d_i d_j); strong(i)
 * lists those columns in CSR order.
 * Aggregation, sequential in ascending row order, aggregates numbered in order of creation. Pass 1: row i is skipped if it is
 * aggregated or any j of strong(i) is; otherwise i and all of strong(i) form the next aggregate. Pass 2, from a copy of pass 1's map:
 * an unaggregated i joins the pass-1 aggregate of the first j of strong(i), in CSR order, that pass 1 aggregated. Pass 3: an i still
 * unaggregated founds the next aggregate with every j of strong(i) still unaggregated at that moment. The members of an aggregate
 * are its rows in ascending order.
 * Coarsest level: level l is the coarsest if rows_l <= 64, or l + 1 = max_levels, or the aggregation of level l gives
 * 10 n_c > 9 rows_l (that aggregation is discarded).
 * Coarse operator A_c = P^T A P, P piecewise constant: row I holds one entry per distinct aggregate J = agg(col) met in its members'
 * rows, sorted by ascending J, stored zeros kept; each value a plain sequential sum that starts from its first term and walks the
 * members in ascending order, each member's entries in CSR order.
 * Per level: lambda_max by the symmetric Gershgorin bound; the smoother is the Chebyshev application of degree nu on
 * [lambda_max / 4.0, lambda_max]; the coarsest level is solved by degree 8 on [lambda_max / 30.0, lambda_max] from a zero guess.
 * Products: level 0 is the operator's own run_device in whatever variant it currently runs; every other level the general CSR product
 * in the automatic variant of that level's matrix.
 * Cycle: steps (1) to (5) of spmv_amd_precond_create_multigrid's text with  (2) r_c[I] = (((t_m0 + t_m1) + t_m2) + ...) over the
 * members of I in ascending order, t_i = fma(-1.0, s_i, r_i), s_i the chain s = +0.0 ; s = fma(v[k], z[col[k]], s) for ascending k --
 * for every row, whatever variant the level's product runs;  (4) z_i = fma(2.0, e_c[agg(i)], z_i): the factor stays 2.0.
 * Limitation: the near-null vector is assumed constant. A symmetric diagonal scaling S A S of a good system coarsens badly from the
 * second level on (the piecewise-constant P no longer fits); a caller-supplied near-null vector is not available. */
SpmvAmdPrecond* spmv_amd_precond_create_amg(SpmvOperator* op, int smoother_degree, int max_levels, double strength, int* bad_row);
/* A handle of spmv_amd_precond_create_amg: the number of levels, nu, theta, the host wall time of the whole creation in ms, and up to
 * cap entries per level: rows, stored entries, the largest aggregate (0 on the coarsest level) and lambda_max. Returns the number of
 * levels, 0 for any other handle (nothing is written). Any out pointer may be NULL. */
int spmv_amd_precond_amg_info(const SpmvAmdPrecond* m, int* levels, int* smoother_degree, double* strength, int* rows, long long* nnz,
                              int* max_aggregate, double* lambda_max, double* setup_ms, int cap);
/* Kind "multigrid" for up to max_rhs (1..8) right-hand sides at once (csrc/multigrid_multi.hip): it is
 * spmv_amd_precond_create_multigrid in every respect -- levels, coarse operators, dinv, Gershgorin bounds, coefficients, refusals, *bad_row --
 * and in addition its hierarchy holds block vectors of max_rhs row-interleaved columns (element (row, column j) at [row * k + j]) on every
 * level above 0 (R, D, Z and W = A Z; level 0 works on the vectors of the solve or of the application) and one SpMM plan per level, on the
 * level's own view and launch variant. max_rhs outside 1..8 is refused before any HIP call like the other arguments. Everything is sized
 * against the device's free memory first; a refusal leaves no device memory behind. The handle is also a complete single-vector multigrid
 * handle: spmv_amd_pcg_solve_device, spmv_amd_precond_apply_device, ..._multigrid_info and ..._multigrid_dimension work on it, bit for
 * bit as on a handle of spmv_amd_precond_create_multigrid. This creator makes the 2-D hierarchy of "stencil5-csr": "stencil7-csr" is
 * refused here as by the 2-D creator; the 3-D hierarchy with block vectors is spmv_amd_precond_create_multigrid3d_multi's. */
SpmvAmdPrecond* spmv_amd_precond_create_multigrid_multi(SpmvOperator* op, int smoother_degree, int max_levels, int max_rhs, int* bad_row);
/* The same for "stencil7-csr" (csrc/multigrid3d_multi.hip): it is spmv_amd_precond_create_multigrid3d in every
 * respect -- levels, coarse operators, dinv, bounds, coefficients, refusals and their order, *bad_row --, with max_rhs outside 1..8
 * refused before any HIP call, and in addition its hierarchy holds the block vectors R, D, Z and W of max_rhs row-interleaved columns on
 * every level above 0 and one SpMM plan per level ("spmm/csr", the kind of the operator's own multi-RHS plan), their bytes sized with
 * everything else against the device's free memory before anything is allocated. Per column the batched cycle is steps (1) to (5) of
 * spmv_amd_precond_create_multigrid3d's text element for element: every row of every product is the CSR loop, the coarse sum runs in
 * the order (((((((t000 + t001) + t010) + t011) + t100) + t101) + t110) + t111) over the members that exist, the correction is
 * z = fma(2.0, e_c[agg(i)], z). The handle is also a complete single-vector 3-D handle: spmv_amd_pcg_solve_device,
 * spmv_amd_precond_apply_device, ..._multigrid_info and ..._multigrid_dimension (3) work on it, bit for bit as on a handle of
 * spmv_amd_precond_create_multigrid3d. */
SpmvAmdPrecond* spmv_amd_precond_create_multigrid3d_multi(SpmvOperator* op, int smoother_degree, int max_levels, int max_rhs, int* bad_row);
/* The same for "cusparse-csr" (csrc/amg_multi.hip): it is spmv_amd_precond_create_amg in every respect -- the
 * argument checks and their sentences, the order of the refusals, *bad_row, the host set-up and every level's aggregates, CSR, dinv,
 * lambda_max and coefficients bit for bit --, with max_rhs outside 1..8 refused before any HIP call beside the other argument checks,
 * and in addition its hierarchy holds the block vectors R, D, Z and W of max_rhs row-interleaved columns on every level above 0 and one
 * SpMM plan per level ("spmm/csr", the kind of the operator's own multi-RHS plan), their bytes sized with everything else against the
 * device's free memory before anything is allocated; a refusal leaves no device memory behind.
 * Per column the batched cycle is steps (1) to (5) of spmv_amd_precond_create_amg's text element for element, with EVERY level's product
 * the sequential chain s = +0.0 ; s = fma(v[k], z[col[k]], s) for ascending k -- what "spmm/csr" computes; the coarse sum runs
 * ((t_m0 + t_m1) + ...) over the members in ascending order, t = fma(-1.0, s, r); the correction is z = fma(2.0, e_c[agg(i)], z).
 * A column's bits therefore do not depend on nrhs, on its slot or on the other columns; a NaN in one column reaches no other. They equal
 * the bits of the single-vector AMG handle wherever level 0 and every coarse level run "csr/stream" or "csr/row-scalar". On a level that
 * runs "csr/adaptive" or "csr/wavefront" (long rows) the single handle sums a row as a tree, and the two agree to rounding only -- the
 * statement the operator's own SpMM makes against its SpMV. The restriction's residual is the sequential chain in both.
 * The handle is also a complete single-vector AMG handle: spmv_amd_pcg_solve_device, spmv_amd_gcr_solve_device,
 * spmv_amd_precond_apply_device, ..._amg_info, ..._multigrid_info and ..._multigrid_dimension (0) work on it, bit for bit as on a handle
 * of spmv_amd_precond_create_amg. The batched PCG, the batched GCR(m) and spmv_amd_precond_apply_device_multi accept it for
 * nrhs <= max_rhs; spmv_amd_bicgstab_solve_device_multi refuses kind "multigrid" as before. */
SpmvAmdPrecond* spmv_amd_precond_create_amg_multi(SpmvOperator* op, int smoother_degree, int max_levels, double strength, int max_rhs,
                                                  int* bad_row);
/* The capacity max_rhs of a handle of the three creators above; 0 for NULL, for another kind and for a handle of
 * spmv_amd_precond_create_multigrid, ..._multigrid3d or ..._amg. */
int spmv_amd_precond_multigrid_max_rhs(const SpmvAmdPrecond* m);
/* Z = M^-1 R on device blocks of nrhs (1..8) row-interleaved columns of n rows (16-byte aligned), for every kind the batched solver
 * accepts: "none" (copy), "jacobi", "chebyshev", and "multigrid" from spmv_amd_precond_create_multigrid_multi,
 * ..._multigrid3d_multi or ..._amg_multi (there per column the bits its own text states) with nrhs <= max_rhs. The checks are those of spmv_amd_precond_apply_device, plus nrhs and the capacity, all before any HIP call ([PCG-MULTI] sentences;
 * "chebyshev" and "multigrid" need the operator's multi-RHS path). d_R is only read; d_Z must not overlap it. Work vectors that are not
 * the hierarchy's live for the call only. Synchronises. Column j of d_Z has exactly the bits spmv_amd_precond_apply_device gives for
 * column j alone: both run the operator's own product bits and the same element-wise fma forms (the fused row-lds step of the single
 * path against SpMM + step kernel here). Returns 0, non-zero for a refusal. */
int spmv_amd_precond_apply_device_multi(SpmvOperator* op, const SpmvAmdPrecond* m, int nrhs, const double* d_R, double* d_Z);
/* z = M^-1 r on device vectors of n rows (16-byte aligned), any kind (none: copy, jacobi: dinv*r). d_z must not overlap d_r, which is
 * only read. rz (may be NULL): r.z summed by the solver's own fixed-shape reduction. The pair (op, m) is checked as by
 * spmv_amd_pcg_solve_device, before any HIP call. Work vectors live for the call only. Synchronises. Returns 0, non-zero for a refusal. */
int spmv_amd_precond_apply_device(SpmvOperator* op, const SpmvAmdPrecond* m, const double* d_r, double* d_z, double* rz);
void spmv_amd_precond_destroy(SpmvAmdPrecond* m);
/* "none", "jacobi", "chebyshev", "multigrid"; "invalid" for NULL. */
const char* spmv_amd_precond_kind(const SpmvAmdPrecond* m);
/* Host copy of dinv (n must be the preconditioner's size); non-zero for kind "none". */
int spmv_amd_precond_inverse_diagonal(const SpmvAmdPrecond* m, double* out, int n);
/* Preconditioned CG on the device. b, x: host arrays of mat->rows values, x in = x0, out = solution (uploaded before and
 * downloaded after the timed region). Refused: NULL pointers, an uninitialised or non-square operator, n != mat->rows, a
 * preconditioner made from another operator or from an earlier init of this one. The workspace (x, b, r, p, Ap; kind
 * "chebyshev": d, z and a second z as well; kind "multigrid" keeps its level vectors in the preconditioner) is sized against the device's free memory first, kept between calls and released with cg_solve_device's (an operator's free(),
 * spmv_amd_cg_release_workspace(), spmv_amd_pcg_release_workspace()). */
int spmv_amd_pcg_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, const double* b, double* x,
                              const CGConfig* config, CGStats* stats);
/* ||r_k||, k = 0..iterations, of the last preconditioned solve (spmv_amd_cg_last_history is not touched by one). */
int spmv_amd_pcg_last_history(double* out, int cap);
/* Releases the solver workspaces: the same as spmv_amd_cg_release_workspace(). Safe to call at any time. */
void spmv_amd_pcg_release_workspace(void);

/* ---- BiCGSTAB: nonsymmetric systems (csrc/bicgstab.hip) ----
 * Right-preconditioned BiCGSTAB over any operator with run_device: A need not be symmetric or definite. The contract is
 * spmv_amd_pcg_solve_device's: b, x host arrays (x in = x0, out = solution; upload and download outside the timed region), the
 * statistics, timer rule and verbose semantics (lines tagged [BICGSTAB-DEVICE]), the stopping rule (strict ||r|| / ||r0|| < tol on
 * the recurrence residual, which right preconditioning keeps the true one; the converging iteration counted), every argument
 * check before the first HIP call with a [BICGSTAB] sentence on stderr and a non-zero return, the pair (op, m) checked as there.
 * m: kind "none" or "jacobi" (a handle of spmv_amd_precond_create_from_diagonal included); kinds "chebyshev" and "multigrid" are
 * built for symmetric definite matrices and refused. A hat means "times dinv" (kind "none": the same vector); every fma is
 * explicit, every other operation rounds once; every dot product is a streaming sum of the PCG shape (pair-wise partials per
 * wave, then pcg_reduce_kernel's geometry), so every operator that gives the same A p bits gives the same solve bits.
 *   r = fma(1.0, b, -1.0 * (A x0)) ; r^ = r ; p = r ; p^ = dinv p ; rho = r.r ; ||r0|| = sqrt(rho) ; history[0] = ||r0||
 *   iteration:
 *   1. v = A p^
 *   2. sigma = r^.v ; zero or not finite: BREAKDOWN -- the iteration is counted, the unchanged residual recorded, nothing updated
 *   3. alpha = rho / sigma ; s = fma(-alpha, v, r) ; s^ = dinv s ; ||s|| = sqrt(s.s)
 *   4. ||s|| / ||r0|| < tol: HALF STEP -- x = fma(alpha, p^, x), the iteration counted, ||s|| recorded, converged
 *   5. t = A s^ ; omega = (t.s) / (t.t) ; t.t or t.s zero or not finite: BREAKDOWN -- x = fma(alpha, p^, x), r = s, ||s||
 *      recorded, the iteration counted
 *   6. x = fma(omega, s^, fma(alpha, p^, x)) ; r = fma(-omega, t, s) ; ||r|| = sqrt(r.r) recorded, the iteration counted, then the
 *      stopping test
 *   7. rho' = r^.r ; zero or not finite: BREAKDOWN, x and r keep their update ; else beta = (rho' / rho) * (alpha / omega) ;
 *      rho = rho' ; p = fma(beta, fma(-omega, v, p), r) ; p^ = dinv p
 * A breakdown ends the solve with converged = 0 and x finite; there is no sign test. The same solve twice gives bit-identical x
 * and history. The workspace (x, b, r, r^, p, v, t; "jacobi": p^ and s^ as well) is sized against the device's free memory first,
 * kept between calls and released with the other CG workspaces (an operator's free(), spmv_amd_cg_release_workspace(),
 * spmv_amd_pcg_release_workspace()). */
int spmv_amd_bicgstab_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, const double* b, double* x,
                                   const CGConfig* config, CGStats* stats);
/* The recorded residual norms, k = 0..iterations, of the last BiCGSTAB solve (the other solvers' histories are not touched by one). */
int spmv_amd_bicgstab_last_history(double* out, int cap);

/* ---- GCR(m): nonsymmetric systems under ANY preconditioner (csrc/gcr.hip) ----
 * Restarted GCR (generalised conjugate residuals; mathematically FGMRES) over any operator with run_device: A need not be symmetric
 * or definite, and m may be of EVERY kind -- "none", "jacobi" (a handle of spmv_amd_precond_create_from_diagonal included),
 * "chebyshev", "multigrid" of either dimension on its own operator: the loop is flexible, so an application that is a polynomial or
 * a V-cycle is as good as a matrix, and it minimises the residual over its basis, so the recorded norm never grows. Kind "chebyshev"
 * is built on the interval of a symmetric definite spectrum: on a convection-dominated matrix the loop does not diverge but MAY
 * STAGNATE (relative residuals of 0.1 .. 0.9 after 1 500 iterations were seen on the CPU); "multigrid" is the preconditioner this
 * solver exists for. The contract is spmv_amd_pcg_solve_device's: b, x host arrays (x in = x0, out = solution; upload and download
 * outside the timed region), the statistics, timer rule and verbose semantics (lines tagged [GCR-DEVICE]), the stopping rule (strict
 * ||r|| / ||r0|| < tol on the recurrence residual, which right preconditioning keeps the true one; the converging iteration
 * counted), every argument check before the first HIP call with a [GCR] sentence on stderr and a non-zero return, the pair (op, m)
 * checked as there. restart = m: 1 .. 32, 0 means the default 16; anything else is refused. Every fma is explicit, every other
 * operation rounds once; every dot product is a streaming sum of the PCG shape (pair-wise partials per wave, then
 * pcg_reduce_kernel's geometry), so an operator contributes only the bits of A z.
 *   r = fma(1.0, b, -1.0 * (A x0)) ; ||r0|| = sqrt(r.r) ; history[0] = ||r0||
 *   iteration k, slot j = k mod m (j == 0 empties the basis):
 *   1. z = M^-1 r      "none": z is r ; "jacobi": dinv * r ; "chebyshev": the application stated above (u = dinv r, d = c0 u, z = d,
 *                      then the steps) ; "multigrid": one V-cycle
 *   2. q = A z
 *   3. beta_i = (q.Q_i) / gamma_i, i = 0 .. j-1, ALL from the q of step 2 (classical Gram-Schmidt: one pass over the basis)
 *   4. for i ascending: q = fma(-beta_i, Q_i, q) ; z = fma(-beta_i, Z_i, z)
 *   5. gamma = q.q ; rho = r.q ; gamma zero or not finite, or rho zero or not finite: BREAKDOWN -- the iteration counted, the
 *      unchanged residual recorded, x untouched, converged = 0
 *   6. alpha = rho / gamma ; x = fma(alpha, z, x) ; r = fma(-alpha, q, r) ; ||r|| = sqrt(r.r) recorded, the iteration counted, then
 *      the strict stopping test
 *   7. Z_j = z ; Q_j = q ; gamma_j = gamma
 * The same solve twice gives bit-identical x and history. The workspace -- x, b, r, 2 m basis vectors, the partials (32 values wide
 * whatever m, so a unit of restart costs its two vectors and nothing else), "jacobi": one vector, "chebyshev": three; a multigrid
 * kind keeps its vectors in the handle -- is sized against the device's free memory first (a request that does not fit is refused
 * with a sentence that names the largest restart that would), kept between calls and released with the other CG workspaces (an
 * operator's free(), spmv_amd_cg_release_workspace(), spmv_amd_pcg_release_workspace()). */
int spmv_amd_gcr_solve_device(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int restart, const double* b, double* x,
                              const CGConfig* config, CGStats* stats);
/* The recorded residual norms, k = 0..iterations, of the last GCR solve (the other solvers' histories are not touched by one). */
int spmv_amd_gcr_last_history(double* out, int cap);
/* The bytes of the vectors and partials a GCR solve of `rows` rows keeps at this restart (0: the default) under this kind ("none",
 * "jacobi", "chebyshev", "multigrid"): (3 + 2 m + s) * 8 * rows + 32 * 8 * ((rows / 2 + 63) / 64, at least 1), s = 0, 1, 3, 0. The
 * history, the scalar record and the reduction scratch (under 100 KB + 8 * max_iters) are not counted. 0: refused arguments (rows
 * < 1, restart outside 0 .. 32, a null or unknown kind). No HIP call. */
size_t spmv_amd_gcr_workspace_bytes(int rows, int restart, const char* kind);

/* ---- preconditioned CG for several right-hand sides (csrc/pcg_multi.hip) ----
 * nrhs (1..8) INDEPENDENT preconditioned solves on one operator under one preconditioner of kind "none", "jacobi" (a from-diagonal one
 * included), "chebyshev", or "multigrid" from spmv_amd_precond_create_multigrid_multi or ..._multigrid3d_multi with nrhs <= max_rhs: per column exactly the algebra, stopping rule and breakdown rule of spmv_amd_pcg_solve_device, with the
 * arguments, statistics, timers and verbose semantics of spmv_amd_cg_solve_device_multi (B, X: host, nrhs vectors of mat->rows values
 * one after the other, X in = x0; stats: nrhs records; verbose lines tagged [PCG-MULTI j]). Only the SpMM and dinv are shared: the
 * operator must have the multi-RHS path ("stencil5-csr" in every variant, "stencil7-csr", "cusparse-csr").
 * Per column j and iteration, element-wise with explicit fma() and one rounding per other operation:
 *   Ap = A p (the SpMM: the single-vector path's bits); pAp = p.Ap; an unusable pAp (zero or not finite): alpha = 0, nothing is updated
 *   and the column stops with converged = 0; else alpha = rz / pAp; r = fma(-alpha, Ap, r); ||r|| = sqrt(r.r), counted and recorded; the
 *   strict test ||r|| / ||r0|| < tol; else z = M^-1 r ("none": r; "jacobi": dinv * r; "chebyshev": u = dinv * r; d = c0 * u; z = d, then
 *   for s = 1..degree: w = A z; d = fma(g_s, dinv * fma(-1.0, w, r), h_s * d); z = z + d); an unusable r.z stops the column with
 *   converged = 0; else beta = r.z / rz, rz = r.z; x = fma(alpha, p, x); p = fma(beta, p, z) unless the column stopped in this iteration.
 * A dot product of column j is the sum of the ROUNDED products per row: 256 consecutive rows per partial (64-lane shuffle trees, then
 * ((w0 + w1) + w2) + w3; p.Ap: the SpMM's own workgroups), 4096 partials per slice (thread t of 256 adds t, t + 256, ... in ascending
 * order, then a 256-wide tree), the slice sums the same way. Every value of column j has the same bits whatever nrhs is and whatever
 * slot the column sits in, and with kind "none" a solve without a breakdown has the bits of spmv_amd_cg_solve_device_multi. (The
 * single-RHS spmv_amd_pcg_solve_device sums in another shape: the two agree to rounding, not bit for bit.)
 * Kind "multigrid": z = one V(nu, nu) cycle, steps (1)-(5) of spmv_amd_precond_create_multigrid's text (a 3-D hierarchy: of
 * ..._multigrid3d's) element for element, per column
 * the algebra of spmv_amd_pcg_solve_device with that kind, the dot products in the shape above. Unlike the single-RHS loop there is no
 * host read before the cycle; the iteration has the "chebyshev" shape: SpMM, step 1, the r update (which writes term 0 of level 0 into D
 * and Z), the verdict, the rest of the cycle, beta, the x / p update, the one read of the column records. In the iteration in which the
 * last column stops the cycle's launches still go out and each returns at once: every kernel of the cycle reads the column records and
 * does nothing when no column is running. A column's bits depend neither on nrhs nor on its slot. Cycle launches that carry an SpMM (the
 * smoothing products, the residual restriction) count as SpMV time under detailed timers, the others as BLAS1.
 * A column that has converged or broken down is frozen: from the next iteration on nothing changes a bit of its x, history or count
 * (kind "multigrid": of its X, R, P, history, count and record; D, Z and the hierarchy's level vectors are scratch for stopped columns).
 * Refused before the first HIP call, with a [PCG-MULTI] sentence on stderr and a non-zero return: nrhs outside 1..8, a NULL
 * argument, max_iters < 0, an operator without the multi-RHS path or used before init, a system that is not square or not of
 * mat->rows rows, kind "multigrid" from spmv_amd_precond_create_multigrid or ..._multigrid3d (its hierarchy holds single vectors: the
 * block creators ..._multigrid_multi and ..._multigrid3d_multi make the batched form), nrhs above a block hierarchy's max_rhs (the sentence names both), a preconditioner of another size, of another operator or
 * from before the operator's last init or free. The workspace (X, R, P, AP; "chebyshev": D and Z too; partials, column records,
 * histories) is sized against the device's free memory first and refused with a sentence if it does not fit; it is kept between
 * calls and released with the other CG workspaces (an operator's free(), spmv_amd_cg_release_workspace(),
 * spmv_amd_pcg_release_workspace()). */
int spmv_amd_pcg_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int nrhs, const double* B, double* X,
                                    const CGConfig* config, CGStats* stats);
/* Residual history of column `rhs` of the last batched preconditioned solve; -1 if there is no such column. */
int spmv_amd_pcg_last_history_multi(int rhs, double* out, int cap);
/* Device bytes the batched preconditioned solver's workspace holds now: 0 once it is released or before the first such solve. No
 * HIP call. */
size_t spmv_amd_pcg_multi_workspace_bytes(void);

/* ---- BiCGSTAB for several right-hand sides (csrc/bicgstab_multi.hip) ----
 * nrhs (1..8) INDEPENDENT BiCGSTAB solves on one operator under one preconditioner of kind "none" or "jacobi" (a from-diagonal one
 * included): per column exactly the algebra of spmv_amd_bicgstab_solve_device -- its steps 1-7, the half step, the three breakdowns
 * (sigma, omega, rho'), the strict stopping test and what each of them records --, with the arguments, statistics, timers and verbose
 * semantics of spmv_amd_pcg_solve_device_multi (B, X: host, nrhs vectors of mat->rows values one after the other, X in = x0; stats:
 * nrhs records; verbose lines tagged [BICGSTAB-MULTI j], the breakdown line naming the scalar as the single solver's does). Not a
 * block Krylov method: every column has its own rho, alpha, omega, beta, verdict, history and iteration count; only the SpMM (two per
 * iteration, each reading the coefficients once for all columns) and one dinv[row] per row are shared. The operator must have the
 * multi-RHS path ("stencil5-csr" in every variant, "stencil7-csr", "cusparse-csr").
 * A dot product of column j is the sum of the ROUNDED products per row in the shape spmv_amd_pcg_solve_device_multi states (256
 * consecutive rows per partial, 4096 partials per slice, the slice sums the same way), every one of them on the vector kernels' own
 * 256-row workgroups. Every value of column j therefore has the same bits whatever nrhs is and whatever slot the column sits in. (The
 * single-RHS spmv_amd_bicgstab_solve_device sums streaming fma chains: the two agree to rounding, not bit for bit.)
 * A column that has converged or broken down is frozen: in the iteration in which it stops it receives exactly the update the single
 * solver applies (nothing, the half step, or the whole step) while the others go on, and from the next iteration on nothing changes a
 * bit of its X, R, r^0, P, P^, history or count; V, T and S^ are scratch for stopped columns. A NaN or inf in one column never reaches
 * another column.
 * Refused before the first HIP call, with a [BICGSTAB-MULTI] sentence on stderr and a non-zero return: nrhs outside 1..8, a NULL
 * argument, max_iters < 0, an operator without the multi-RHS path or used before init, a system that is not square or not of
 * mat->rows rows, kinds "chebyshev" and "multigrid" (block hierarchies included: built for symmetric definite matrices), a
 * preconditioner of another size, of another operator or from before the operator's last init or free. The workspace (block vectors X,
 * R, r^0, P, V, T; "jacobi": P^ and S^ too; partials for two values, slices, column records, histories) is sized against the device's
 * free memory first and refused with a sentence if it does not fit; it is kept between calls and released with the other CG
 * workspaces (an operator's free(), spmv_amd_cg_release_workspace(), spmv_amd_pcg_release_workspace()). */
int spmv_amd_bicgstab_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int nrhs, const double* B, double* X,
                                         const CGConfig* config, CGStats* stats);
/* Residual history of column `rhs` of the last batched BiCGSTAB solve; -1 if there is no such column (the other solvers' histories
 * are not touched by one). */
int spmv_amd_bicgstab_last_history_multi(int rhs, double* out, int cap);
/* Device bytes the batched BiCGSTAB solver's workspace holds now: 0 once it is released or before the first such solve. No HIP call. */
size_t spmv_amd_bicgstab_multi_workspace_bytes(void);

/* ---- GCR(m) for several right-hand sides (csrc/gcr_multi.hip) ----
 * nrhs (1..8) INDEPENDENT restarted GCR solves on one operator under one preconditioner of ANY kind -- "none", "jacobi" (a
 * from-diagonal one included), "chebyshev", and "multigrid" on a hierarchy with block vectors (spmv_amd_precond_create_multigrid_multi,
 * ..._multigrid3d_multi) of at least nrhs columns: per column exactly the algebra of spmv_amd_gcr_solve_device -- its steps 1-7,
 * classical Gram-Schmidt from the q of the product, i ascending in step 4, the breakdown rule (gamma or rho zero or not finite: x
 * untouched, the iteration counted, the unchanged residual recorded), the strict stopping test and what each of them records --, with
 * the arguments, statistics, timers and verbose semantics of spmv_amd_pcg_solve_device_multi (B, X: host, nrhs vectors of mat->rows
 * values one after the other, X in = x0; stats: nrhs records; verbose lines tagged [GCR-MULTI j], the breakdown line naming the scalar
 * as the single solver's does). restart: 1..32, or 0 for the default 16. Not a block Krylov method: every column has its own basis,
 * gammas, betas, alpha, verdict, history and iteration count; the running columns are in the same iteration and so share the slot
 * j = iteration mod restart. Only the SpMM, one dinv[row] per row and the preconditioner's block application are shared. The
 * operator must have the multi-RHS path ("stencil5-csr" in every variant, "stencil7-csr", "cusparse-csr").
 * A dot product of column j is the sum of the ROUNDED products per row in the shape spmv_amd_pcg_solve_device_multi states (256
 * consecutive rows per partial, 4096 partials per slice, the slice sums the same way). Every value of column j therefore has the same
 * bits whatever nrhs is and whatever slot the column sits in. (The single-RHS spmv_amd_gcr_solve_device sums streaming fma chains:
 * the two agree to rounding, not bit for bit.)
 * A column that has converged or broken down is frozen: from the next iteration on nothing changes a bit of its X, R, history, count
 * or record; its basis slots and the application's vectors are scratch. A NaN or inf in one column never reaches another column.
 * Refused before the first HIP call, with a [GCR-MULTI] sentence on stderr and a non-zero return: nrhs outside 1..8, restart outside
 * 0..32, a NULL argument, max_iters < 0, an operator without the multi-RHS path or used before init, a system that is not square or
 * not of mat->rows rows, a "multigrid" handle whose hierarchy keeps single vectors or fewer than nrhs columns, a preconditioner of
 * another size, of another operator or from before the operator's last init or free. The workspace (block vectors X, R, the
 * transfer vector, "jacobi": dinv r, "chebyshev" and "multigrid": D and Z; 2 x restart basis block vectors, allocated slot by slot;
 * partials for 32 values, slices, column records, histories) is sized against the device's free memory first and refused with a
 * sentence that names the largest restart that fits; it is kept between calls and released with the other CG workspaces (an
 * operator's free(), spmv_amd_cg_release_workspace(), spmv_amd_pcg_release_workspace()). */
int spmv_amd_gcr_solve_device_multi(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, int restart, int nrhs, const double* B,
                                    double* X, const CGConfig* config, CGStats* stats);
/* Residual history of column `column` of the last batched GCR solve; -1 if there is no such column (the other solvers' histories are
 * not touched by one). */
int spmv_amd_gcr_last_history_multi(int column, double* out, int cap);
/* The bytes of the block vectors and partials a batched GCR solve of nrhs systems of `rows` rows keeps at this restart (0: the
 * default) under this kind ("none", "jacobi", "chebyshev", "multigrid"): (4 + 2 x restart) block vectors, two more for "chebyshev" and
 * "multigrid", and 32 x nrhs partial rows. One unit of restart costs exactly 16 x rows x nrhs bytes. 0 for refused arguments. No HIP
 * call. */
size_t spmv_amd_gcr_multi_workspace_bytes(int rows, int nrhs, int restart, const char* kind);

/* ---- multi-GPU communicator ---- */
typedef struct SpmvAmdComm SpmvAmdComm;

/* Host-side callbacks of a staged communicator: the library moves the halo rows
 * and the scalars through pinned host memory and calls these on host buffers
 * (the reference's D2H -> MPI -> H2D scheme, cg_solver_mgpu_partitioned.cu:173-231).
 * A NULL send/recv pointer means "no neighbour on that side". */
typedef int (*SpmvAmdHostHaloFn)(void* user, const double* send_prev, const double* send_next,
                                 double* recv_prev, double* recv_next, int count);
typedef int (*SpmvAmdHostAllreduceFn)(void* user, double* inout, int count);
/* root receives counts[r] doubles at displs[r] of recv; every rank sends send[0..n_send). */
typedef int (*SpmvAmdHostGatherFn)(void* user, const double* send, int n_send, double* recv,
                                   const int* counts, const int* displs);
typedef int (*SpmvAmdHostBarrierFn)(void* user);

/* 256-byte blob (two RCCL unique ids: one communicator for the halo send/recv, one for
 * the all-reduces), to be produced on rank 0 and handed to every rank. */
#define SPMV_AMD_COMM_ID_BYTES 256
int spmv_amd_comm_unique_id(void* out_id256);
/* One process per GPU: RCCL communicator over xGMI; halo rows travel by
 * ncclSend/ncclRecv on a side stream, dot products by ncclAllReduce. */
/* Returns NULL if RCCL cannot create the communicators. */
SpmvAmdComm* spmv_amd_comm_create_rccl(int rank, int world, const void* id256);
SpmvAmdComm* spmv_amd_comm_create_staged(int rank, int world, SpmvAmdHostHaloFn halo,
                                         SpmvAmdHostAllreduceFn allreduce,
                                         SpmvAmdHostGatherFn gather, SpmvAmdHostBarrierFn barrier,
                                         void* user);
void spmv_amd_comm_destroy(SpmvAmdComm* comm);
/* The communicator cg_solve_mgpu_partitioned runs over (MPI_COMM_WORLD's role). */
void spmv_amd_comm_set_world(SpmvAmdComm* comm);
int spmv_amd_comm_rank(const SpmvAmdComm* comm);
int spmv_amd_comm_size(const SpmvAmdComm* comm);
/* Runs one all-reduce (value rank+1 on every rank -> world*(world+1)/2), one neighbour exchange
 * (64 doubles carrying the sender's rank, both ways) and one barrier through the communicator and
 * checks what arrived; 0 on success. Collective: every rank must call it. */
int spmv_amd_comm_selftest(SpmvAmdComm* comm);
/* All ranks meet (reference: MPI_Barrier, cg_solver_mgpu_partitioned.cu:405). Like every wait on another
 * rank in this library it is bounded by the watchdog: after SPMV_AMD_WATCHDOG_S seconds (default 60,
 * 0 = unbounded) without progress the rank reports where it is stuck and exits with EXIT_FAILURE. */
int spmv_amd_comm_barrier(SpmvAmdComm* comm);
/* "rccl", "staged" or "self"; and the number of ranks the device transport itself reports
 * (ncclCommCount of both RCCL communicators; 0 for transports without such a notion). */
const char* spmv_amd_comm_transport(const SpmvAmdComm* comm);
int spmv_amd_comm_transport_ranks(const SpmvAmdComm* comm);

/* ---- peer-mailbox all-reduce (optional; csrc/comm.hpp) ----
 * The two dot-product all-reduces per CG iteration (reference: MPI_Allreduce on the host,
 * cg_solver_mgpu_partitioned.cu:583,645) as direct stores between the GPUs of one node: every rank owns a small
 * mailbox in uncached device memory that all ranks map through hipIpc. spmv_amd_comm_mailbox_enable() does the
 * whole set-up over the communicator's own transport (collective; returns 1 when EVERY rank has a mailbox that
 * passed a self-test of 2048 checked all-reduces, else 0 and the communicator keeps all-reducing through RCCL / the staged callbacks).
 * The three steps are also available one by one for callers that exchange the handles themselves. */
#define SPMV_AMD_MAILBOX_HANDLE_BYTES 64
int spmv_amd_comm_mailbox_enable(SpmvAmdComm* comm);
int spmv_amd_comm_mailbox_prepare(SpmvAmdComm* comm, void* handle_out64);
int spmv_amd_comm_mailbox_connect(SpmvAmdComm* comm, const void* all_handles, int count);
int spmv_amd_comm_mailbox_selftest(SpmvAmdComm* comm, int rounds);
void spmv_amd_comm_mailbox_disable(SpmvAmdComm* comm);
int spmv_amd_comm_mailbox_ready(const SpmvAmdComm* comm);

/* ---- resident multi-GPU CG (what cg_solve_mgpu_partitioned is built from) ---- */
typedef struct SpmvAmdCgSlab SpmvAmdCgSlab;

/* Slab of a host matrix: build_csr_struct + slice + upload, as the reference does. */
SpmvAmdCgSlab* spmv_amd_cg_slab_create(MatrixData* mat, SpmvAmdComm* comm);
/* Slab of the synthetic n x n stencil, generated in HBM; b = 1, x0 = 0. */
SpmvAmdCgSlab* spmv_amd_cg_slab_create_stencil5(int n, SpmvAmdComm* comm);
/* Full-length host vectors as in the reference (each rank uploads its slab);
 * NULL keeps b = 1 / x0 = 0. While no x0 was ever passed, x0 holds the zeros the library wrote itself and most loads of it are
 * skipped (csrc/cg_slab.hpp, x0_known_zero): the flush of x in ring mode does not read it, and on a slab without neighbours that
 * owns its matrix, in ring mode, the first SpMV reads it on the grid's first and last grid row only. Where, besides, every row of the
 * matrix sums to +0.0 over zero operands (every stored coefficient finite and one per row with its sign bit clear: checked once at
 * creation) and the slab's SpMV runs on block tiles, r0 = b - A x0 is b bit for bit and no launch computes it: the first launch of a
 * solve is iteration 0's SpMV on b, which also sums b.b, and b stands in for the first direction buffer; b is never written. Slabs
 * with neighbours and the in-place form (ring 1) still read x0 in the first SpMV, and a solve of no iterations copies it into x.
 * SPMV_AMD_ZERO_START=0 at creation: always loaded, r0 always computed. A passed x0 is never inspected, zeros included. Results are
 * bit-identical either way. */
int spmv_amd_cg_slab_set_vectors(SpmvAmdCgSlab* s, const double* b_full, const double* x0_full);
/* One solve from the stored x0; the timed region is the reference's
 * (cg_solver_mgpu_partitioned.cu:405-413 -> 728-731).
 * The loop has two shapes (csrc/slab_decisions.hpp, LoopShape), bit-identical in their results. PIPELINE (default on a slab with
 * neighbours): the halo exchange runs on a side stream under the interior rows' SpMV; the boundary rows wait inside their
 * launch for a device flag the side stream raises behind the receive, and the side stream's exchange waits for a device
 * flag the direction update's first workgroups raise. CONCURRENCY REQUIREMENT: those two waits spin (bounded: 20 s, or half of
 * SPMV_AMD_WATCHDOG_S) for a kernel on the OTHER stream, so the two streams' kernels must be able to run at the same time --
 * true on the hardware queues of a normal process, NOT under a tool that serialises dispatches (rocprofv3 --pmc): run such
 * passes with SPMV_AMD_NO_OVERLAP=1. PLAIN (SPMV_AMD_NO_OVERLAP=1 read at creation, detailed timers, the in-place form, slabs too
 * thin to split): everything on the compute stream, the exchange behind the whole direction update, the reference's own order
 * (:680-703); no device flag, no spin. A wait that gives up ends the process with the watchdog's sentence on stderr. */
int spmv_amd_cg_slab_solve(SpmvAmdCgSlab* s, const CGConfigMultiGPU* config,
                           CGStatsMultiGPU* stats);
/* Which shape this slab's loop takes and who decided (a static string): "single rank"; "single rank: direction update inside the
 * block SpMV" (a rank without neighbours that owns its matrix, direction ring > 1, a whole-slab launch on block tiles whose
 * row-by-row blocks are at most 1/16 of its blocks, SPMV_AMD_FUSED_DIRECTION not 0: the direction update p' = r + beta p of
 * iteration k is evaluated inside the SpMV launch of iteration k + 1; a solve with detailed timers keeps the two launches; where
 * every row of block tiles of that launch is evaluated either all by the fast path or all row by row, and SPMV_AMD_AP_RECOMPUTE is
 * not 0, that launch does not store A p' on the fast blocks and the r update recomputes it from p', same bits -- and, unless
 * SPMV_AMD_FIRST_RECOMPUTE is 0, iteration 0 does the same with A p0, recomputed from b or from the stored r0; such a slab's block tiles
 * hold 8 grid rows unless SPMV_AMD_ROWLDS_BLOCK_ROWS says 0, 4 or 8, every other slab's hold 4); "pipeline (verified against the plain
 * order at creation)"; "plain: SPMV_AMD_NO_OVERLAP=1"; "plain: the in-place form (ring 1) or a slab too thin to split"; "plain: the
 * pipeline's residual history differed from the plain order's in the creation check". The creation check: the first slab created on a communicator that exchanges halos solves four iterations
 * in each shape (default b = 1, x0 = 0); the shapes are bit-identical by construction, so a difference on any rank -- lost or stale
 * halo rows, a device flag that never comes -- makes every slab on that communicator run the plain order, with a line on
 * stderr. Set-up work, once per communicator, outside every timed region. */
const char* spmv_amd_cg_slab_loop_shape(const SpmvAmdCgSlab* s);
/* Gathers the solution into x_full on rank 0 (other ranks get their own slab). */
int spmv_amd_cg_slab_gather(SpmvAmdCgSlab* s, double* x_full);
int spmv_amd_cg_slab_history(SpmvAmdCgSlab* s, double* out, int cap);
/* Slab-local SpMV on caller data: uploads x_full's slab + halos, returns y slab. */
int spmv_amd_cg_slab_spmv(SpmvAmdCgSlab* s, const double* x_full, double* y_local);
void spmv_amd_cg_slab_info(const SpmvAmdCgSlab* s, int* row_offset, int* n_local, int* local_nnz);
/* The SpMV kernel variant the slab's solver launches ("stencil5/row-lds", ...): a static string. */
const char* spmv_amd_cg_slab_variant(const SpmvAmdCgSlab* s);
/* Average duration (HIP events on the solver's stream) of `reps` launches of the
 * slab SpMV kernel pair on the current direction vector. */
int spmv_amd_cg_slab_time_spmv(SpmvAmdCgSlab* s, int reps, float* ms_each);
/* Per-rank timeline of a solve: what the reference reports as max / min of six timers per rank
 * (cg_solver_mgpu_partitioned.cu:748-800), taken here WITHOUT the per-stage host syncs its detailed timers need:
 * with the timeline on, a solve records HIP events at the stage boundaries of every iteration (compute stream) and
 * around every halo exchange (side stream) and resolves them after the loop, so the overlap of the exchange with the
 * interior rows stays as it is in a timed solve. spmv_amd_cg_slab_timeline() returns the values of the last such
 * solve -- averages per counted iteration, microseconds -- in the order of the comma-separated names
 * spmv_amd_cg_slab_timeline_names() returns; 0 values if the last solve ran without the timeline. Each stage runs from
 * the end of the previous stage's last kernel to the end of its own, so queue gaps are inside the stage that waits.
 * (Since round 5 the scalar step of the RCCL path runs inside the direction update's launch: the stage named
 * "reduce_rr_allreduce_and_scalar_step" then holds the sum and the all-reduce only.)
 * Every event record is a barrier packet on the stream (~6 us on MI355X): a solve with the timeline on is ~40 us per iteration
 * slower than a plain one and its small stages consist mostly of that packet (profiles/r05_slab_timeline_p8.txt).
 * The direction-update stage is averaged over the launches that did work ("direction_updates": the converging
 * iteration's update is never needed -- the reference tests convergence before its p update, :652-676). */
void spmv_amd_cg_slab_set_timeline(SpmvAmdCgSlab* s, int on);
/* Placement at creation (csrc/cg_slab_create.hip). Slabs of >= 16 Mi rows place their coefficient stream by timing up to three
 * allocations one region apart: {0, candidates timed, SpMV ms before, SpMV ms kept}. Returns 4, or 0 if it did not run.
 * Addresses only: results never change; a candidate that does not fit ends the trial, never the process. */
int spmv_amd_cg_slab_placement(const SpmvAmdCgSlab* s, double* out, int cap);
/* Row-lds tiles per XCD and run, timed at creation on slabs of >= 16 Mi rows (csrc/device_runtime.hpp, tune_rowlds_xcd_run):
 * {rule, kept, SpMV ms with the rule, ms kept}. Returns 4, or 0 if the trial did not run. Workgroup -> tile mapping only. */
int spmv_amd_cg_slab_tile_runs(const SpmvAmdCgSlab* s, double* out, int cap);
/* Wall ms of creation's set-up phases, each closed by a device synchronisation; none of it lies inside a timed region (the
 * reference builds and uploads before its own, cg_solver_mgpu_partitioned.cu:303-413): {matrix to HBM (upload or generation),
 * streams + vectors, verification + launch plans, coefficient placement trial, tile-run trial}. Returns 5. */
int spmv_amd_cg_slab_setup_ms(const SpmvAmdCgSlab* s, double* out, int cap);
/* The coefficients the slab's SpMV streams (csrc/cg_slab.hpp): 0 = its CSR values (40 B/row), 1 = the symmetric planes
 * (24 B/row: C, E and S per row; W and N are the E of row i-1 and the S of row i-n). A slab takes the planes when it owns its
 * matrix, every launch is a row-lds launch and those W / N entries equal their CSR entries bit for bit (checked at creation);
 * the results are the CSR form's, bit for bit. */
int spmv_amd_cg_slab_coefficient_form(const SpmvAmdCgSlab* s);
/* Inside form 1: a row-lds tile (128 columns of one grid row) whose coefficients all equal, bit for bit, one slab-wide quintuple
 * (W, C, E, N, S) -- any constant-coefficient stencil away from perturbed entries -- is evaluated without loading a coefficient;
 * which tiles those are is decided once at creation against the CSR values (one byte per tile). *total = the tiles of the slab's
 * grid rows that are evaluated from the planes (global grid rows 1 .. n-2), *uniform = how many of them load no coefficient.
 * Both 0 for a slab in form 0. Either pointer may be null. Returns 0. Results are the CSR form's, bit for bit. */
int spmv_amd_cg_slab_uniform_tiles(const SpmvAmdCgSlab* s, long long* uniform, long long* total);
/* The timed in-loop SpMV launches of the last solve, one by one (ms, iteration order). Returns their number. */
int spmv_amd_cg_slab_spmv_launch_ms(const SpmvAmdCgSlab* s, float* out, int cap);
const char* spmv_amd_cg_slab_timeline_names(void);
int spmv_amd_cg_slab_timeline(const SpmvAmdCgSlab* s, double* out, int cap);
void spmv_amd_cg_slab_destroy(SpmvAmdCgSlab* s);

/* write_matrix_market_stencil5 with other value texts (e.g. "-4.0", "-1.0": the convention
 * of the shipped matrix/example81x81.mtx); used to regenerate test fixtures. */
int spmv_amd_write_stencil5_values(int n, const char* filename, const char* center_text,
                                   const char* off_text);

/* Library build string ("libspmv_amd <date> gfx950 ..."). */
const char* spmv_amd_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_AMD_API_H */
