/* lab.h -- entry points of the LAB build only (cuda-spmv-benchmark_amd/lib/libspmv_amd_lab.so: the product's sources compiled
 * with -DSPMV_AMD_LAB). Test and measurement hooks: tests/, tools/ and bench.py's one-GPU scaling probe load that library;
 * the product library (libspmv_amd.so, include/spmv_amd/api.h) neither exports these symbols nor reads the environment
 * switches listed here -- the reference has no such switches either (include/spmv.h:46-64: errors exit, nothing else).
 *
 * Environment switches the LAB build reads in addition to the product's (each ONCE, at creation):
 *   SPMV_AMD_SELF_NEIGHBOUR=1, SPMV_AMD_FORCE_COLLECTIVES=1   a single RCCL rank as its own neighbour / issuing its all-reduces
 *   SPMV_AMD_TEST_WEDGE_OVERLAPPED_EXCHANGE=1 | 2 | 3 | 4     fault injection: the side-stream exchange never returns on the
 *                                                             host | the overlapped pipeline delivers a nudged system | the rows
 *                                                             of a side-stream exchange never travel | its arrival flag never comes
 *   SPMV_AMD_PLACEMENT_FAIL_AFTER=k                           the k-th further placement candidate "does not fit"
 */
#ifndef SPMV_AMD_LAB_H
#define SPMV_AMD_LAB_H

#include "spmv_amd/api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stand-in slab: the slab rank `as_rank` of an `as_world`-GPU run would own (same rows, CSR bytes, halo length and
 * neighbour sides; reference partition, cg_solver_mgpu_partitioned.cu:259-268,306-331), carried by ONE rank whose
 * communicator was created under SPMV_AMD_SELF_NEIGHBOUR=1 and exchanges the halo rows with itself through the transport's
 * own send / recv path: the previous-rank halo receives the slab's own first grid row, the next-rank halo its last (the slab
 * mirrored at its cuts, not the global system). Timing of the real per-rank shapes on one GPU, and the oracle test of the
 * RCCL hand-overs (tests/test_distributed.py). */
SpmvAmdCgSlab* spmv_amd_cg_slab_create_stencil5_as(int n, int as_rank, int as_world, SpmvAmdComm* comm);

/* Options of an existing slab (A/B runs on the same allocations): "no_overlap" 0/1 (1 = the PLAIN loop shape: halo exchange on
 * the compute stream behind the whole direction update), "late_bulk" 0 / 1 / 2 (off / the lead-status-rest protocol in EVERY
 * iteration / only where the known residual says convergence is near: the default rule on slabs of >= 1e8 rows), "lead_rows" N, "run_ahead" 0 / 1 / 2
 * (1, the default: the host runs one iteration ahead of the status records while the known residual is far from the tolerance;
 * 2: test hook, every iteration is guessed "far", so each solve learns of its convergence one iteration late) --
 * results are bit-identical under each --, "spmv_event_stride" N (time every N-th in-loop SpMV launch; default 7, phase advancing with every solve; 0 = none),
 * and the one option that is NOT result-neutral, a timing aid for stand-in slabs: "stop_at" K (iteration K counts as the
 * converging one whatever its residual; 0 = off), and "csr_coefficients" 0/1 (1 = the SpMV streams the CSR values even where the
 * slab holds the symmetric planes, spmv_amd_cg_slab_coefficient_form; results are bit-identical) and "stream_coefficients" 0/1
 * (1 = the kernel ignores the tile class map and streams the planes on every tile, spmv_amd_cg_slab_uniform_tiles; composes with
 * "csr_coefficients"; results are bit-identical), "block_rows" 0 / 4 / 8 (grid rows per block tile of the in-loop SpMV, the
 * product's SPMV_AMD_ROWLDS_BLOCK_ROWS; 0 = the one-row kernel; the block maps are rebuilt; results are bit-identical) and
 * "spmv_with_dot" 0/1 (1 = spmv_amd_cg_slab_spmv runs the SpMV in its in-loop form, p.Ap partials and their sum included, so that
 * it takes the kernel the loop takes), and "fused_direction" 0 / 1 / 2 (the product's SPMV_AMD_FUSED_DIRECTION: 0 = the direction
 * update is a launch of its own, 1 = it rides in the next block SpMV's launch where the slab is eligible -- one rank, ring > 1, no
 * detailed timers, a block map whose slow blocks are at most 1/16 of its blocks --, 2 = the same without the 1/16 cap;
 * spmv_amd_cg_slab_loop_shape says which ran; results are bit-identical) and "zero_start" 0/1 (the product's SPMV_AMD_ZERO_START:
 * 0 = the first SpMV and the flush of x always load x0 and the first launch stores r0 twice; spmv_amd_cg_slab_initial_stage says
 * which form a solve takes; results are bit-identical) with "zero_start_parts" 0..15 (a field of the LAB build only: which parts "zero_start" 1 switches on, for A/B
 * runs of each: 1 = the first launch without x loads, 2 = r0 stored once, 4 = the flush of x without x0, 8 = b serves as p0 and
 * iteration 0's SpMV sums b.b, spmv_amd_cg_slab_first_stage; default 15), "ap_recompute" 0/1 (the product's SPMV_AMD_AP_RECOMPUTE: 1 = in
 * iterations >= 1 of the fused direction loop the fused launch does not store A p' on its fast blocks and the r update recomputes
 * it from p' on skewed block tiles, where every row block of the whole-slab block map is all-fast or all-slow;
 * spmv_amd_cg_slab_ap_form says which ran; results are bit-identical) and "direction_store" 0/1 (a field of the LAB build only: 0 =
 * spmv_amd_cg_slab_direction_spmv runs the fused launch in the form that does not store A p'), "first_recompute" 0/1 (the product's
 * SPMV_AMD_FIRST_RECOMPUTE: 1 = where "ap_recompute" applies, iteration 0 takes the same form -- its SpMV does not store A p0 on the
 * fast blocks and its r update recomputes it from the one vector that is both r0 and p0; spmv_amd_cg_slab_first_recompute_form says
 * which ran; results are bit-identical) and "first_store" 0/1 (a field of the LAB build only: 0 = spmv_amd_cg_slab_first_stage, and
 * spmv_amd_cg_slab_spmv in its in-loop form, run the launch that does not store A x on the fast blocks; y is NaN there). Returns 0,
 * or -1 for an unknown name or value. */
int spmv_amd_cg_slab_set_option(SpmvAmdCgSlab* s, const char* name, long long value);

/* The tile class map of a slab in the symmetric form as creation wrote it (spmv_amd_cg_slab_uniform_tiles): one byte per row-lds
 * tile at [local grid row * ceil(n / 128) + column tile], 1 = uniform, 0 = the tile streams the planes (the grid's first and last
 * grid row, which walk the CSR, hold 0). Copies min(count, cap) bytes to `out` (host) and returns count; 0 = no map. */
long long spmv_amd_cg_slab_tile_classes(const SpmvAmdCgSlab* s, unsigned char* out, long long cap);

/* The block map of one launch range of the in-loop SpMV (which = 0: the whole slab; 1: the rows that need no halo): one byte per
 * block tile -- 128 columns x block_rows grid rows counted from the range's first grid row -- at [row block * ceil(n / 128) +
 * column tile], 1 = every tile of the block is uniform and the block holds block_rows rows (the fast path), 0 = the block is
 * evaluated row by row. Copies min(count, cap) bytes to `out` (host) and returns count; 0 = the range has no map. */
long long spmv_amd_cg_slab_block_map(const SpmvAmdCgSlab* s, int which, unsigned char* out, long long cap);

/* The slow blocks of a launch range (which: as above): the indices of the block tiles whose map byte is 0, ascending -- what the
 * launch behind the direction update inside the block SpMV evaluates, one workgroup each. Copies min(count, cap) ints to `out`
 * (host) and returns count. */
long long spmv_amd_cg_slab_slow_blocks(const SpmvAmdCgSlab* s, int which, int* out, long long cap);

/* What the last spmv_amd_cg_slab_spmv in its in-loop form ("spmv_with_dot" 1) left beside y on a slab without neighbours: *pAp = the
 * reduced x . (A x), and the whole-slab launch's partials, one per 128 x 1 tile (min(count, cap) doubles to `partials`; returns count). */
int spmv_amd_cg_slab_spmv_dot(const SpmvAmdCgSlab* s, double* pAp, double* partials, int cap);

/* The direction update inside the block SpMV alone, once, on the caller's r and p_in (host, n_local doubles each): the fused launch,
 * the launch over the slow blocks and the reduction, as an iteration >= 1 of that loop shape enqueues them, with beta as the
 * device scalar. iteration_matches = 0: the launches are handed another iteration number than the scalars hold; converged != 0: the
 * scalars say the solve is over -- in both cases every launch must return on the scalars. p_out, Ap (n_local doubles), partials
 * (up to cap doubles) and *pAp are NaN wherever a launch did not write. Returns the number of partials the launches write, or -1 on
 * a slab that cannot take the launch (neighbours, ring 1, no block map). */
int spmv_amd_cg_slab_direction_spmv(SpmvAmdCgSlab* s, const double* r, const double* p_in, double beta, int iteration_matches, int converged,
                                    double* p_out, double* Ap, double* pAp, double* partials, int cap);

/* The r update of an iteration >= 1 alone, once, on the caller's vectors (host, n_local doubles each) and scalars (alpha = rr_old /
 * pAp on the device): recompute = 0, cg_update_r_kernel on (r, Ap); recompute != 0, the launch that recomputes A p' from p_new on
 * the fast row blocks and reads Ap on the slow ones only (csrc/skew_geometry.hpp). reverse != 0: the tiles are walked from the end.
 * converged != 0: the launch must return on the scalars. r_out (n_local doubles) and partials (min(count, cap) doubles, NaN where
 * the launch did not write) come back. Returns the number of partials the launch writes (one per 128 consecutive elements), or -1
 * where recompute is asked of a slab that is not eligible. */
int spmv_amd_cg_slab_update_r_stage(SpmvAmdCgSlab* s, int recompute, int reverse, const double* r, const double* p_new, const double* Ap,
                                    double rr_old, double pAp, int converged, double* r_out, double* partials, int cap);
/* The r update that recomputes A p': bit 0 = a solve would take the form now, bit 1 = the last solve took it, bit 2 = every row block
 * of the whole-slab block map is all-fast or all-slow. *launches (may be NULL) = the recomputing launches the last solve enqueued.
 * s == NULL: the workspace slab of cg_solve_device, which borrows the caller's operator (-1: there is none). */
int spmv_amd_cg_slab_ap_form(const SpmvAmdCgSlab* s, int* launches);

/* Iteration 0's r update alone, once, where r0 and p0 are the one vector src (host, n_local doubles; b or ring slot 0 in a solve):
 * recompute = 0, cg_update_r_from_kernel on (Ap, src); recompute != 0, the out-of-place launch that recomputes A src on the fast row
 * blocks and reads Ap on the slow ones only. reverse, converged, r_out, partials and the return value as in
 * spmv_amd_cg_slab_update_r_stage; r_out is NaN where the launch did not write. src_back (may be NULL, n_local doubles): src as it
 * lies on the device behind the launch. */
int spmv_amd_cg_slab_update_r_from_stage(SpmvAmdCgSlab* s, int recompute, int reverse, const double* src, const double* Ap, double rr_old,
                                         double pAp, int converged, double* r_out, double* src_back, double* partials, int cap);
/* Iteration 0's form that a solve of at least one iteration would take now: 0 = A p0 stored and read back; else left unstored on the
 * fast blocks and recomputed by the r update, 1 = from b (b serves as p0), 2 = from ring slot 0 (r0 stored once), 3 = in place on
 * (r, ring slot 0). *last (may be NULL) = what the last solve took (0 for a solve of no iterations). Counted apart from
 * spmv_amd_cg_slab_ap_form's launches, which are those of iterations >= 1. */
int spmv_amd_cg_slab_first_recompute_form(const SpmvAmdCgSlab* s, int* last);

/* The initial stage of a solve alone, once, on the slab's stored b and x0: the first SpMV's launch (r0 = b - A x0, p0 = r0, one
 * partial of r0.r0 per 128 x 1 tile) and the reduction of the partials, in the form a solve would take now. Returns the form: bit 0 =
 * x0 holds the zeros the library wrote and the launch requests no x value on interior grid rows; bit 1 = r0 is stored once, as p0,
 * and iteration 0's r update reads it there. r0 == NULL: only that, nothing is launched. Otherwise r0 (n_local doubles) = the
 * residual from where it lives, r_vec (n_local doubles, may be NULL) = the r vector, NaN where the launch did not write (all of it
 * with bit 1), partials (min(*count, cap) doubles) and *rr = the reduced sum. -1 on a slab with neighbours or one whose first SpMV
 * does not write the residual. */
int spmv_amd_cg_slab_initial_stage(SpmvAmdCgSlab* s, double* r0, double* r_vec, double* partials, int cap, int* count, double* rr);

/* The first stage of a solve whose p0 is b itself: x0 holds the library's zeros AND every row of the matrix sums to +0.0 over zero
 * operands (every stored coefficient finite, one with its sign bit clear; established at creation), so r0 = b - A 0 is b bit for
 * bit, no launch computes it, and iteration 0's block SpMV on b goes first and also sums b.b. Returns 1 where a solve of at least
 * one iteration would take that shape now (one rank, ring > 1, the block kernel on the whole slab, no detailed timers,
 * "zero_start_parts" bit 8), else 0; with Ap == NULL, or 0, only that: nothing is launched. Otherwise runs, once, on the stored b,
 * what such a solve enqueues -- the launch (tiles walked from the end with reverse != 0), the reduction of the b.b partials, the
 * scalars' initialisation, the reduction of the b.(A b) partials -- and returns Ap (n_local doubles), both partial arrays (min(slots,
 * cap) doubles each, one slot per 128 x 1 tile; NaN where the launch did not write), *count = the slots the launch writes, *rr = b.b
 * and *pAp = b.(A b). The initial stage above keeps launching the kernels it launched before this shape existed. */
int spmv_amd_cg_slab_first_stage(SpmvAmdCgSlab* s, int reverse, double* Ap, double* pAp_partials, double* bb_partials, int cap, int* count,
                                 double* rr, double* pAp);
/* The slab's stored right-hand side as it lies on the device now (n_local doubles): where b serves as p0 the solver reads it in
 * three more places and must never write it. Returns 0. */
int spmv_amd_cg_slab_stored_b(SpmvAmdCgSlab* s, double* b_local);

/* The device scalars of one preconditioned solve (csrc/pcg.hip keeps the same record on the device). */
typedef struct SpmvAmdPcgScalars {
    double rz;        /* r.z of the current residual */
    double pAp, alpha, beta;
    double b_norm;    /* ||r0|| */
    double residual;  /* ||r_k|| */
    int iterations;
    int converged;    /* stopping test met */
    int breakdown;    /* pAp or r.z' zero or not finite: stopped, not converged */
    int skip_update;  /* this iteration's pAp broke down: r and x stay as they are */
} SpmvAmdPcgScalars;

/* Device pointers and sizes of one spmv_amd_pcg_stage call; a stage reads only the fields listed for it. */
typedef struct SpmvAmdPcgStageArgs {
    size_t n;            /* rows (init, update_r, update_xp) */
    const double* b;     /* init */
    const double* Ap;    /* init, update_r */
    const double* dinv;  /* kind "jacobi": init, update_r, update_xp; kind "none": not looked at */
    double* r;           /* init: out; update_r: in and out; update_xp: in */
    double* p;           /* init: out; update_xp: in and out */
    double* x;           /* update_xp: in and out */
    double* partials;    /* init, update_r: out, value v of workgroup g at [v * count + g]; reduce: in, the same layout */
    int count;           /* init, update_r: out, the workgroups of the launch = partials per value ((n / 2 + 63) / 64, at least 1:
                            the buffer holds 2 * count doubles); reduce: in */
    int which;           /* reduce: the scalar step, 0 = initial r.r / r.z, 1 = p.Ap (ONE value), 2 = r.r / r.z' */
    double tol;          /* reduce, which = 2 */
    double* hist;        /* reduce: residual history, hist_cap doubles (may be null when hist_cap is 0) */
    int hist_cap;
} SpmvAmdPcgStageArgs;

/* The preconditioned solver's own kernels (csrc/pcg.hip), one stage per call on the caller's device data -- the launches
 * spmv_amd_pcg_solve_device makes, through the functions it makes them with: same kernels, grid, block size, reduction geometry
 * and stage buffer. The model is spmv_amd_cg_fused_step (api.h); tests/test_pcg_stages_gpu.py holds each stage against the
 * oracle. Every call synchronises. stage (kind = "jacobi" or "none"; "reduce" does not look at it):
 *   "init"       r = b - Ap, z = dinv r ("none": z = r), p = z, the partials of r.r (value 0) and r.z (value 1); sets a->count
 *   "update_r"   r = fma(-alpha, Ap, r) unless scalars->skip_update, z = dinv r in registers, the partials of r.r and r.z;
 *                sets a->count
 *   "update_xp"  nothing when scalars->skip_update; else x = fma(alpha, p, x) and, unless scalars->converged or ->breakdown,
 *                p = fma(beta, p, dinv r) (r and dinv are not read otherwise)
 *   "reduce"     the sums of a->count partials of one (which = 1) or two values, then the scalar step `which` on *scalars (read
 *                and written, all ten fields) with a->tol, a->hist and a->hist_cap
 * Vectors are accessed in 16-byte pairs. Refused before any HIP call, with a sentence on stderr and a non-zero return: an
 * unknown stage or kind, null arguments, n < 1, count < 1, which outside 0..2, hist_cap < 0, a null pointer the stage needs
 * (scalars: every stage but "init"), a vector that is not 16-byte aligned, partials or hist that are not 8-byte aligned.
 * Returns 0 otherwise. */
int spmv_amd_pcg_stage(const char* stage, const char* kind, SpmvAmdPcgStageArgs* a, SpmvAmdPcgScalars* scalars);

/* The device scalars of one BiCGSTAB solve (csrc/bicgstab.hip keeps the same record on the device; api.h states the algebra). */
typedef struct SpmvAmdBicgstabScalars {
    double rho;       /* r^.r of the current residual */
    double sigma, alpha, omega, beta;
    double b_norm;    /* ||r0|| */
    double residual;  /* the norm recorded last */
    double s_norm;    /* ||s|| of this iteration */
    int iterations;
    int converged;    /* stopping test met (by the half step or by the whole one) */
    int breakdown;    /* 0, or which scalar stopped the solve: 1 sigma, 2 omega (t.t or t.s), 3 rho' */
    int x_step;       /* what the x / r kernel applies in this iteration: 0 nothing, 1 the half step, 2 the whole step */
    int stop;         /* the verdict: set with converged or breakdown; kernels behind it return at once */
    int pad;
} SpmvAmdBicgstabScalars;

/* Device pointers and sizes of one spmv_amd_bicgstab_stage call; a stage reads only the fields listed for it. Kind "none" keeps
 * p^ in p and s^ in r: phat and shat are not looked at. */
typedef struct SpmvAmdBicgstabStageArgs {
    size_t n;            /* rows (every stage but reduce) */
    const double* b;     /* init */
    const double* dinv;  /* kind "jacobi": init, update_s, direction */
    double* x;           /* update_xr: in and out */
    double* r;           /* init: out; update_s: in (r) and out (s); dot_t: in (s); update_xr: in (s) and out (r); direction: in */
    double* rhat;        /* init: out; dot_rv, update_xr: in */
    double* p;           /* init: out; direction: in and out; kind "none": update_xr: in */
    double* phat;        /* kind "jacobi": init, direction: out; update_xr: in */
    double* shat;        /* kind "jacobi": update_s: out; update_xr: in */
    double* v;           /* init: in (A x0); dot_rv, update_s, direction: in */
    const double* t;     /* dot_t, update_xr: in */
    double* partials;    /* the vector stages: out, value v of workgroup g at [v * count + g]; reduce: in, the same layout */
    int count;           /* the vector stages: out, the workgroups of the launch = partials per value ((n / 2 + 63) / 64, at least 1:
                            the buffer holds 2 * count doubles); reduce: in */
    int which;           /* reduce: the scalar step, 0 = r0.r0, 1 = sigma = r^.v, 2 = s.s, 3 = t.s / t.t (two values), 4 = r.r / r^.r
                            (two values) */
    double tol;          /* reduce, which = 2 and 4 */
    double* hist;        /* reduce: residual history, hist_cap doubles (may be null when hist_cap is 0) */
    int hist_cap;
} SpmvAmdBicgstabStageArgs;

/* The BiCGSTAB solver's own kernels (csrc/bicgstab.hip), one stage per call on the caller's device data -- the launches
 * spmv_amd_bicgstab_solve_device makes, through the functions it makes them with. The model is spmv_amd_pcg_stage;
 * tests/test_bicgstab_stages_gpu.py holds each stage against the restatement. Every call synchronises. stage (kind = "jacobi" or
 * "none"; "reduce", "dot_rv" and "dot_t" do not look at it):
 *   "init"       r = fma(1.0, b, -1.0 * v), r^ = r, p = r, p^ = dinv p, the partials of r.r; sets a->count
 *   "dot_rv"     the partials of r^.v; sets a->count
 *   "update_s"   nothing when scalars->stop; else r = fma(-alpha, v, r) (now s), s^ = dinv s, the partials of s.s; sets a->count
 *   "dot_t"      nothing when scalars->stop; else the partials of t.s (value 0) and t.t (value 1), s read from r; sets a->count
 *   "update_xr"  scalars->x_step 0: nothing; 1: x = fma(alpha, p^, x); 2: x = fma(omega, s^, fma(alpha, p^, x)), r = fma(-omega, t, r)
 *                and the partials of r.r (value 0) and r^.r (value 1); sets a->count
 *   "direction"  nothing when scalars->stop; else p = fma(beta, fma(-omega, v, p), r), p^ = dinv p
 *   "reduce"     the sums of a->count partials of one (which 0..2) or two values, then the scalar step `which` on *scalars (read and
 *                written, every field) with a->tol, a->hist and a->hist_cap
 * Vectors are accessed in 16-byte pairs. Refused before any HIP call, with a sentence on stderr and a non-zero return: an unknown
 * stage or kind, null arguments, n < 1, count < 1, which outside 0..4, hist_cap < 0, a null pointer the stage needs (scalars: every
 * stage but "init" and "dot_rv"), a vector that is not 16-byte aligned, partials or hist that are not 8-byte aligned. Returns 0
 * otherwise. */
int spmv_amd_bicgstab_stage(const char* stage, const char* kind, SpmvAmdBicgstabStageArgs* a, SpmvAmdBicgstabScalars* scalars);

/* The device scalars of one GCR solve (csrc/gcr.hip keeps the same record on the device; api.h states the algebra). */
#define SPMV_AMD_GCR_MAX_RESTART 32
#define SPMV_AMD_GCR_DOT_CHUNK 8   /* basis vectors per chunk of the multidot kernel */
#define SPMV_AMD_GCR_ORTH_CHUNK 4  /* basis slots per chunk of the orthogonalise kernel */
typedef struct SpmvAmdGcrScalars {
    double gamma[SPMV_AMD_GCR_MAX_RESTART]; /* q.q of the basis slots filled since the last restart */
    double beta[SPMV_AMD_GCR_MAX_RESTART];  /* this iteration's (q.Q_i) / gamma_i, i < slot */
    double alpha, rho;                      /* this iteration's step length and r.q */
    double b_norm;                          /* ||r0|| */
    double residual;                        /* the norm recorded last */
    int iterations;
    int converged;
    int breakdown; /* 0, or which scalar stopped the solve: 1 gamma = q.q, 2 rho = r.q */
    int stop;      /* the verdict: set with converged or breakdown; kernels behind it return at once */
} SpmvAmdGcrScalars;

/* Device pointers and sizes of one spmv_amd_gcr_stage call; a stage reads only the fields listed for it. Q and Z are HOST arrays of
 * device pointers, one 16-byte aligned vector per basis slot; entries past `slot` are not looked at. */
typedef struct SpmvAmdGcrStageArgs {
    size_t n;            /* rows (every stage but reduce) */
    const double* b;     /* init */
    const double* v;     /* init: A x0 */
    const double* dinv;  /* kind "jacobi": init, update_xr */
    double* x;           /* update_xr: in and out */
    double* r;           /* init: out; orthogonalise: in; update_xr: in and out */
    double* zs;          /* kind "jacobi": init, update_xr: out, dinv r */
    const double* z_in;  /* orthogonalise: z = M^-1 r (may be r itself) */
    double* const* Q;    /* multidot: Q[0 .. slot] in; orthogonalise: Q[0 .. slot-1] in, Q[slot] in and out; update_xr: Q[slot] in */
    double* const* Z;    /* orthogonalise: Z[0 .. slot-1] in, Z[slot] out; update_xr: Z[slot] in */
    int slot;            /* j: multidot 1 .. 31, orthogonalise and update_xr 0 .. 31; reduce: which = 1 and 2 */
    double* partials;    /* the vector stages: out, value v of workgroup g at [v * count + g]; reduce: in, the same layout */
    int count;           /* the vector stages: out, the workgroups of the launch = partials per value ((n / 2 + 63) / 64, at least 1);
                            reduce: in */
    int which;           /* reduce: the scalar step, 0 = r0.r0, 1 = the betas (slot values), 2 = gamma and rho (two values), 3 = r.r */
    double tol;          /* reduce, which = 3 */
    double* hist;        /* reduce: residual history, hist_cap doubles (may be null when hist_cap is 0) */
    int hist_cap;
} SpmvAmdGcrStageArgs;

/* The GCR solver's own kernels (csrc/gcr.hip), one stage per call on the caller's device data -- the launches
 * spmv_amd_gcr_solve_device makes, through the functions it makes them with. The model is spmv_amd_bicgstab_stage;
 * tests/test_gcr_stages_gpu.py holds each stage against the restatement. Every call synchronises. stage (kind = "jacobi" or "none";
 * "multidot", "orthogonalise" and "reduce" do not look at it):
 *   "init"           r = fma(1.0, b, -1.0 * v), "jacobi": zs = dinv r, the partials of r.r; sets a->count
 *   "multidot"       nothing when scalars->stop; else the partials of Q[i].Q[slot], value i = 0 .. slot-1; sets a->count
 *   "orthogonalise"  nothing when scalars->stop; else for i ascending below slot q = fma(-beta[i], Q[i], q), z = fma(-beta[i], Z[i], z)
 *                    from q = Q[slot], z = z_in; Q[slot] = q (not written at slot 0), Z[slot] = z, the partials of q.q (value 0) and
 *                    r.q (value 1); sets a->count
 *   "update_xr"      nothing when scalars->stop; else x = fma(alpha, Z[slot], x), r = fma(-alpha, Q[slot], r), "jacobi": zs = dinv r,
 *                    the partials of r.r; sets a->count
 *   "reduce"         the sums of a->count partials of one (which 0, 3), slot (which 1) or two (which 2) values, then the scalar step
 *                    `which` on *scalars (read and written, every field) with a->tol, a->hist and a->hist_cap; which >= 1 does nothing
 *                    when scalars->stop
 * Vectors are accessed in 16-byte pairs. Refused before any HIP call, with a sentence on stderr and a non-zero return: an unknown
 * stage or kind, null arguments, n < 1, a slot outside the stage's range, count < 1, which outside 0..3, hist_cap < 0, a null pointer
 * the stage needs (scalars: every stage but "init"), a vector that is not 16-byte aligned, partials or hist that are not 8-byte
 * aligned. Returns 0 otherwise. */
int spmv_amd_gcr_stage(const char* stage, const char* kind, SpmvAmdGcrStageArgs* a, SpmvAmdGcrScalars* scalars);

/* Kind "chebyshev": how many step launches of the last solve's LOOP did work, i.e. were not stopped by the iteration's verdict (the
 * application behind the initial residual is not counted). Every iteration but the converging one runs `degree` of them:
 * degree * (iterations - 1) for a solve that converged. 0 after a solve of another kind. */
int spmv_amd_pcg_last_step_launches(void);

/* Kind "multigrid" (csrc/multigrid.hip): the V-cycles the last solve's LOOP ran (the one behind the initial residual is not counted):
 * iterations - 1 for a solve that converged, iterations for one that reached max_iters. 0 after a solve of another kind. */
int spmv_amd_pcg_last_multigrid_cycles(void);
/* One level's CSR (rows + 1, nnz, nnz values: a complete 5-point stencil of the level's grid, spmv_amd_precond_multigrid_info; a complete
 * 7-point one of n_l^3 rows and 7 n_l^3 - 6 n_l^2 entries where spmv_amd_precond_multigrid_dimension is 3) and dinv (rows) copied to the host; any out pointer may be NULL. Non-zero for another kind or a level that does not exist. */
int spmv_amd_precond_multigrid_level_csr(const SpmvAmdPrecond* m, int level, int* row_ptr, int* col_idx, double* values, double* dinv);
/* Device pointers of one spmv_amd_mg_stage call; n = the FINE grid, the coarse grid is (n + 1) / 2. The 3-D stages read the same record:
 * the CSR is then a complete 7-point stencil of n^3 rows, the vectors hold n^3 and ((n + 1) / 2)^3 values. */
typedef struct SpmvAmdMgStageArgs {
    int n;
    const int* row_ptr;      /* coarsen, residual_restrict: the fine level's CSR, a complete 5-point stencil of grid n (checked) */
    const int* col_idx;
    const double* values;
    double* z;               /* residual_restrict: in; prolong: in and out (16-byte aligned) */
    const double* r;         /* residual_restrict: in (16-byte aligned) */
    double* coarse;          /* residual_restrict: out, r_c; prolong: in, e_c (8-byte aligned) */
    int* out_row_ptr;        /* coarsen: the coarse CSR, out */
    int* out_col_idx;
    double* out_values;
} SpmvAmdMgStageArgs;
/* The multigrid cycle's own launches, one per call on the caller's device data, through the functions the cycle makes them with.
 * Every call synchronises. stage: "coarsen" (A_c = P^T A P), "residual_restrict" (r_c = P^T (r - A z) in one launch), "prolong"
 * (z = fma(2.0, e_c[agg(i)], z)); "coarsen3d", "residual_restrict3d", "prolong3d": the same three of a 3-D level
 * (csrc/multigrid3d.hip), with the 7-point structure check. Refused before any HIP call: an unknown stage, null arguments, n outside
 * 2..46340 (a 3-D stage: 2..674), a null or misaligned pointer the stage needs; after the structure check: a CSR that is not the
 * complete stencil. Returns 0 otherwise. */
int spmv_amd_mg_stage(const char* stage, SpmvAmdMgStageArgs* a);

/* Device pointers and sizes of one spmv_amd_amg_stage call (csrc/amg.hip). */
typedef struct SpmvAmdAmgStageArgs {
    int rows;                /* fine rows */
    int cols;                /* residual_restrict: the length of z (the columns of the CSR) */
    int coarse_rows;         /* aggregates: the length of the coarse vector */
    const int* row_ptr;      /* residual_restrict: the fine level's CSR, rows + 1 / nnz / nnz */
    const int* col_idx;
    const double* values;
    const int* agg_ptr;      /* residual_restrict: coarse_rows + 1 */
    const int* members;      /* residual_restrict: agg_ptr[coarse_rows] fine rows; a row no aggregate lists is never read */
    const int* agg;          /* prolong_correct: rows aggregates */
    double* z;               /* residual_restrict: in (8-byte aligned); prolong_correct: in and out (16-byte aligned) */
    const double* r;         /* residual_restrict: in */
    double* coarse;          /* residual_restrict: out, r_c; prolong_correct: in, e_c */
} SpmvAmdAmgStageArgs;
/* The two launches an AMG level adds to the cycle, one per call on the caller's device data, through the functions the cycle makes
 * them with. Every call synchronises. stage: "residual_restrict" (r_c[I] = ((t_m0 + t_m1) + ...) over the members of I, one launch) or
 * "prolong_correct" (z = fma(2.0, e_c[agg[i]], z)). Refused before any HIP call: an unknown stage, null arguments, sizes below 1, a
 * null or misaligned pointer the stage needs. The index arrays are then read back and checked on the host -- row_ptr ascending from
 * 0, columns in [0, cols), agg_ptr ascending from 0, members in [0, rows), agg in [0, coarse_rows) --: an index outside its range is
 * refused before the launch. Returns 0 otherwise. */
int spmv_amd_amg_stage(const char* stage, SpmvAmdAmgStageArgs* a);
/* The same two launches on block vectors of k (1..8) row-interleaved columns (csrc/amg_multi.hip), on the same
 * record: z holds cols x k (residual_restrict) or rows x k (prolong_correct) values, r rows x k, coarse coarse_rows x k, element
 * (row, column j) at [row * k + j]; every column is running. z, r and coarse are 8-byte aligned, 16-byte where k is even. The checks
 * and the host-side index validation before the launch are spmv_amd_amg_stage's (one body, csrc/amg.hip), plus k. */
int spmv_amd_amg_multi_stage(const char* stage, int k, SpmvAmdAmgStageArgs* a);
/* The aggregate of every row of one level of an AMG hierarchy (spmv_amd_precond_amg_info has the rows) copied to the host; the level's
 * CSR and dinv come from spmv_amd_precond_multigrid_level_csr. Non-zero for another handle, a level that does not exist or the
 * coarsest level, which has no aggregates. */
int spmv_amd_precond_amg_level_aggregates(const SpmvAmdPrecond* m, int level, int* agg);

/* Per-column state of a batched CG solve (csrc/multi_rhs.hpp keeps the same record on the device, one per column). */
typedef struct SpmvAmdMultiColumn {
    double rr_old;    /* r.r of the last iteration that did not converge */
    double pAp, alpha, beta;
    double b_norm;    /* ||r0|| */
    double residual;  /* ||r_k|| */
    int active;       /* the column takes part in the current iteration (the pAp step sets it: !done) */
    int done;         /* converged: frozen from the next iteration on */
    int iterations;
    int pad;
} SpmvAmdMultiColumn;

/* Device pointers and sizes of one spmv_amd_cg_multi_stage call; a stage reads only the fields listed for it. Block vectors
 * are row-interleaved, k columns: element (row, column j) at [row * k + j] (api.h, spmv_amd_spmm_device). */
typedef struct SpmvAmdCgMultiStageArgs {
    const char* mode;          /* spmm: the operator's name ("stencil5-csr", "cusparse-csr"), initialised */
    size_t n;                  /* init, update_r, update_xp: rows */
    double* X;                 /* spmm: in; update_xp: in and out */
    double* R;                 /* init: in (b) and out; update_r: in and out; update_xp: in */
    double* P;                 /* init: out; update_xp: in and out */
    double* AP;                /* spmm: out (A X); init, update_r: in */
    SpmvAmdMultiColumn* cols;  /* update_r, update_xp: in; reduce: in and out -- k records, DEVICE memory */
    double* partials;          /* spmm (may be null: no dot products), init, update_r: out, column j's partial of workgroup g at
                                  [j * count + g]; reduce: in, the same layout */
    long long count;           /* spmm, init, update_r: out, the workgroups of the launch = partials per column (the buffer holds
                                  k * count doubles: the operator's SpMM blocks, (n + 255) / 256 for the vector stages); reduce: in */
    int which;                 /* reduce: the scalar step, 0 = initial r.r, 1 = p.Ap, 2 = r.r */
    double tol;                /* reduce, which = 2 */
    double* hist;              /* reduce: k histories of hist_cap doubles, column j's at [j * hist_cap] (may be null when
                                  hist_cap is 0) */
    int hist_cap;
    int xcd_run;               /* spmm: > 0 replaces the plan's XCD run length for this launch (row-lds looks at it, no other
                                  kind); 0 = the plan's own */
} SpmvAmdCgMultiStageArgs;

/* The batched solver's own kernels (csrc/spmm_kernels.hip, csrc/cg_multi.hip), one stage per call on the caller's device data
 * -- the launches spmv_amd_cg_solve_device_multi makes, through the functions it makes them with, for k = 1..8 columns. The
 * model is spmv_amd_pcg_stage; tests/test_multi_rhs_stages_gpu.py holds each stage against the oracle. Every call
 * synchronises. stage:
 *   "spmm"       AP = A X on the operator `mode`; with partials, the per-column partials of x.(A x); sets a->count to the
 *                plan's workgroups
 *   "init"       R = R - AP (R holds b on entry), P = R, the partials of r.r; sets a->count
 *   "update_r"   r_j = fma(-alpha_j, Ap_j, r_j) for the columns with cols[j].active, the partials of r.r of every column;
 *                sets a->count
 *   "update_xp"  for the columns with cols[j].active: x_j = fma(alpha_j, p_j, x_j) and, unless cols[j].done,
 *                p_j = fma(beta_j, p_j, r_j)
 *   "reduce"     the sums of a->count partials of each column, then the scalar step `which` on cols[j] with a->tol, a->hist and
 *                a->hist_cap (step 0 writes hist[j * hist_cap] unconditionally: it needs hist_cap >= 1, as the solve's
 *                max_iters + 1 is)
 * Refused before any HIP call, with a sentence on stderr and a non-zero return: an unknown stage, k outside 1..8, null
 * arguments, a null pointer the stage needs, n < 1, count < 1, which outside 0..2, hist_cap < 0 (< 1 for step 0), a block vector
 * of a vector stage that is not 16-byte aligned, one of "spmm" that is not 8-byte aligned, partials, cols or hist that are not
 * 8-byte aligned, xcd_run < 0, an operator that is unknown, not initialised or without a multi-RHS path. Returns 0 otherwise. */
int spmv_amd_cg_multi_stage(const char* stage, int k, SpmvAmdCgMultiStageArgs* a);

/* Per-column state of a batched preconditioned solve (csrc/multi_rhs.hpp keeps the same record on the device, one per column):
 * SpmvAmdPcgScalars per column, with the batched loop's two flags. */
typedef struct SpmvAmdPcgMultiColumn {
    double rz;        /* r.z of the column's current residual */
    double pAp, alpha, beta;
    double b_norm;    /* ||r0|| */
    double residual;  /* ||r_k|| */
    int active;       /* the column takes part in the current iteration (step 1: !done) */
    int done;         /* converged or broken down: frozen from the next iteration on */
    int iterations;
    int converged;    /* stopping test met */
    int breakdown;    /* pAp or r.z' zero or not finite: stopped, not converged */
    int skip_update;  /* this iteration's pAp broke down: r and x stay as they are */
    int pad[2];
} SpmvAmdPcgMultiColumn;

/* Device pointers and sizes of one spmv_amd_pcg_multi_stage call; a stage reads only the fields listed for it. Block vectors are
 * row-interleaved, k columns: element (row, column j) at [row * k + j]. */
typedef struct SpmvAmdPcgMultiStageArgs {
    size_t n;                     /* the vector stages: rows */
    double* X;                    /* update_xp: in and out */
    double* R;                    /* init: in (b) and out (r0); update_r: in and out; cheb_step: in; update_xp ("none", "jacobi"): in */
    double* P;                    /* init ("none", "jacobi"): out; update_xp: in and out */
    double* AP;                   /* init, update_r: in; cheb_step: in, W = A Z */
    double* D;                    /* kind "chebyshev": init, update_r: out; cheb_step: in and out */
    double* Z;                    /* kind "chebyshev": init, update_r: out; cheb_step: in and out; update_xp: in */
    const double* dinv;           /* kinds "jacobi" and "chebyshev": n values */
    SpmvAmdPcgMultiColumn* cols;  /* update_r, update_xp, cheb_step: in; reduce: in and out -- k records, DEVICE memory */
    double* partials;             /* init, update_r, cheb_step: out, value v of column j and workgroup g at [(v * k + j) * count + g]
                                     (value 0 = r.r, value 1 = r.z: the buffer holds 2 * k * count doubles); reduce: in, value v of
                                     the step's values at the same place */
    long long count;              /* the vector stages: out, the workgroups of the launch = (n + 255) / 256; reduce: in */
    int which;                    /* reduce: the scalar step, 0 = initial r.r / r.z (two values), 1 = p.Ap, 2 = r.r / r.z' (two values),
                                     3 = r.r and the verdict alone, 4 = r.z' and beta alone (ONE value, at value 0's place) */
    double tol;                   /* reduce, which = 2 or 3 */
    double* hist;                 /* reduce: k histories of hist_cap doubles one after the other (may be null when hist_cap is 0) */
    int hist_cap;
    double c0;                    /* kind "chebyshev": init, update_r: term 0's coefficient */
    double g, h;                  /* cheb_step: the step's coefficients */
    int last;                     /* kind "chebyshev": init, update_r: term 0 is the whole polynomial (the r.z partials are written);
                                     cheb_step: the last step (the r.z partials are written, as value 1) */
} SpmvAmdPcgMultiStageArgs;

/* The batched preconditioned solver's own kernels (csrc/pcg_multi.hip), one stage per call on the caller's device data -- the
 * launches spmv_amd_pcg_solve_device_multi makes, through the functions it makes them with, for k = 1..8 columns. The model is
 * spmv_amd_cg_multi_stage. Every call synchronises. kind: "none", "jacobi" or "chebyshev" ("reduce" does not look at it). stage:
 *   "init"       R = R - AP (R holds b), z = M^-1 r as far as one pass goes ("none": r, "jacobi": dinv r -> P; "chebyshev": term 0
 *                -> D and Z), the partials of r.r and (unless "chebyshev" without `last`) r.z; sets a->count
 *   "update_r"   r = fma(-alpha, AP, r) for the columns with cols[j].active and without skip_update, z as above (kept in registers
 *                for "none" / "jacobi"; D and Z of the active columns for "chebyshev"), the same partials; sets a->count
 *   "cheb_step"  d = fma(g, dinv fma(-1, w, r), h d), z = z + d for the columns with cols[j].done == 0; `last`: the partials of r.z
 *                as value 1; nothing at all once every column is done; sets a->count
 *   "update_xp"  x = fma(alpha, p, x) for the active columns without skip_update, then p = fma(beta, p, z) for those not done
 *   "reduce"     the sums of a->count partials of the step's one or two values per column, then the scalar step `which` on cols
 * Refused before any HIP call, with a sentence on stderr and a non-zero return: an unknown stage or kind, "cheb_step" with another
 * kind than "chebyshev", k outside 1..8, null arguments, n < 1, count < 1, which outside 0..4, hist_cap < 0, a null pointer the
 * stage needs, a block vector that is not 16-byte aligned, dinv, cols, partials or hist that are not 8-byte aligned. Returns 0
 * otherwise. */
int spmv_amd_pcg_multi_stage(const char* stage, const char* kind, int k, SpmvAmdPcgMultiStageArgs* a);

/* Per-column state of a batched BiCGSTAB solve (csrc/multi_rhs.hpp keeps the same record on the device; api.h states the algebra). */
typedef struct SpmvAmdBicgstabMultiColumn {
    double rho;       /* r^.r of the column's current residual */
    double sigma, alpha, omega, beta;
    double b_norm;    /* ||r0|| */
    double residual;  /* the norm recorded last */
    double s_norm;    /* ||s|| of this iteration */
    int active;       /* the column takes part in the current iteration (step 1: !done) */
    int done;         /* converged or broken down: frozen from the next iteration on */
    int iterations;
    int converged;    /* stopping test met (by the half step or by the whole one) */
    int breakdown;    /* 0, or which scalar stopped the column: 1 sigma, 2 omega (t.t or t.s), 3 rho' */
    int x_step;       /* what update_xr applies to the column in this iteration: 0 nothing, 1 the half step, 2 the whole step */
    int pad[2];
} SpmvAmdBicgstabMultiColumn;

/* Device pointers and sizes of one spmv_amd_bicgstab_multi_stage call; a stage reads only the fields listed for it. Block vectors are
 * row-interleaved, k columns: element (row, column j) at [row * k + j]. Kind "none" keeps p^ in P and s^ in R: PH and SH are not
 * looked at. */
typedef struct SpmvAmdBicgstabMultiStageArgs {
    size_t n;                          /* the vector stages: rows */
    double* X;                         /* update_xr: in and out */
    double* R;                         /* init: in (b) and out (r0); update_s: in (r) and out (s); dot_t: in (s); update_xr: in (s) and
                                          out (r); direction: in */
    double* RH;                        /* r^0. init: out; dot_rv, update_xr: in */
    double* P;                         /* init: out; direction: in and out; kind "none": update_xr: in */
    double* PH;                        /* kind "jacobi": init, direction: out; update_xr: in */
    double* SH;                        /* kind "jacobi": update_s: out; update_xr: in */
    double* V;                         /* init: in (A x0); dot_rv, update_s, direction: in */
    double* T;                         /* dot_t, update_xr: in */
    const double* dinv;                /* kind "jacobi": init, update_s, direction: n values */
    SpmvAmdBicgstabMultiColumn* cols;  /* every vector stage but init: in; reduce: in and out -- k records, DEVICE memory */
    double* partials;                  /* the vector stages but direction: out, value v of column j and workgroup g at
                                          [(v * k + j) * count + g] (the buffer holds 2 * k * count doubles); reduce: in, the same layout */
    long long count;                   /* the vector stages: out, the workgroups of the launch = (n + 255) / 256; reduce: in */
    int which;                         /* reduce: the scalar step, 0 = r0.r0, 1 = sigma = r^.v, 2 = s.s, 3 = t.s / t.t (two values),
                                          4 = r.r / r^.r (two values) */
    double tol;                        /* reduce, which = 2 and 4 */
    double* hist;                      /* reduce: k histories of hist_cap doubles one after the other (may be null when hist_cap is 0) */
    int hist_cap;
} SpmvAmdBicgstabMultiStageArgs;

/* The batched BiCGSTAB solver's own kernels (csrc/bicgstab_multi.hip), one stage per call on the caller's device data -- the launches
 * spmv_amd_bicgstab_solve_device_multi makes, through the functions it makes them with, for k = 1..8 columns. The model is
 * spmv_amd_pcg_multi_stage; tests/test_bicgstab_multi_stages_gpu.py holds each stage against numpy. Every call synchronises. kind:
 * "none" or "jacobi" ("reduce", "dot_rv" and "dot_t" do not look at it). A column is RUNNING behind step 1 when cols[j].active and not
 * cols[j].done. stage:
 *   "init"       R = fma(1.0, R, -1.0 * V) (R holds b, V holds A x0), RH = R, P = R, PH = dinv P, the partials of r.r; sets a->count
 *   "dot_rv"     the partials of r^.v for the columns with cols[j].done == 0 (0.0 for the others); nothing at all once every column
 *                is done; sets a->count
 *   "update_s"   for the running columns r = fma(-alpha, v, r) (now s), s^ = dinv s, the partials of s.s (0.0 for the others); sets
 *                a->count
 *   "dot_t"      for the running columns the partials of t.s (value 0) and t.t (value 1), s read from R; sets a->count
 *   "update_xr"  per active column by its x_step -- 0: nothing; 1: x = fma(alpha, p^, x); 2: x = fma(omega, s^, fma(alpha, p^, x)),
 *                r = fma(-omega, t, r) and the partials of r.r (value 0) and r^.r (value 1; 0.0 for every other column); nothing at
 *                all when no column is active; sets a->count
 *   "direction"  for the running columns p = fma(beta, fma(-omega, v, p), r), p^ = dinv p
 *   "reduce"     the sums of a->count partials of the step's one or two values per column, then the scalar step `which` on cols
 * A stage changes no bit of a column it does not name above, also where that column shares a 16-byte pair with one it does; a unit
 * (one or two neighbouring columns of a row) without such a column is not read. Refused before any HIP call, with a sentence on
 * stderr and a non-zero return: an unknown stage or kind, k outside 1..8, null arguments, n < 1, count < 1, which outside 0..4,
 * hist_cap < 0, a null pointer the stage needs, a block vector that is not 16-byte aligned, dinv, cols, partials or hist that are
 * not 8-byte aligned. Returns 0 otherwise. */
int spmv_amd_bicgstab_multi_stage(const char* stage, const char* kind, int k, SpmvAmdBicgstabMultiStageArgs* a);

/* Per-column state of a batched GCR(m) solve (csrc/multi_rhs.hpp keeps the same record on the device; api.h states the algebra). */
#define SPMV_AMD_GCR_MULTI_DOT_CHUNK 4   /* basis slots per chunk of the batched multidot kernel */
#define SPMV_AMD_GCR_MULTI_ORTH_CHUNK 2  /* basis slots per chunk of the batched orthogonalise kernel */
typedef struct SpmvAmdGcrMultiColumn {
    double gamma[SPMV_AMD_GCR_MAX_RESTART]; /* q.q of the basis slots filled since the last restart */
    double beta[SPMV_AMD_GCR_MAX_RESTART];  /* this iteration's (q.Q_i) / gamma_i, i < slot */
    double alpha, rho;
    double b_norm;    /* ||r0|| */
    double residual;  /* the norm recorded last */
    int done;         /* converged or broken down: frozen from then on, this record included */
    int iterations;
    int converged;
    int breakdown;    /* 0, or which scalar stopped the column: 1 gamma = q.q, 2 rho = r.q */
} SpmvAmdGcrMultiColumn;

/* Device pointers and sizes of one spmv_amd_gcr_multi_stage call; a stage reads only the fields listed for it. Block vectors are
 * row-interleaved, k columns: element (row, column j) at [row * k + j]. Q and Z are HOST arrays of SPMV_AMD_GCR_MAX_RESTART device
 * pointers, one block vector per basis slot; slots above `slot` are not looked at. */
typedef struct SpmvAmdGcrMultiStageArgs {
    size_t n;                     /* the vector stages: rows */
    double* X;                    /* update_xr: in and out */
    double* R;                    /* init: in (b) and out (r0); orthogonalise: in; update_xr: in and out */
    const double* AX;             /* init: in, A x0 */
    const double* z_in;           /* orthogonalise: in, where the application left z; may BE R (kind "none") */
    double* ZS;                   /* kind "jacobi": init, update_xr: out, dinv r */
    double** Q;                   /* multidot: Q[0 .. slot] in; orthogonalise: Q[0 .. slot - 1] in, Q[slot] in and out; update_xr: Q[slot] in */
    double** Z;                   /* orthogonalise: Z[0 .. slot - 1] in, Z[slot] out; update_xr: Z[slot] in */
    int slot;                     /* j: multidot 1 .. 31, orthogonalise and update_xr 0 .. 31; reduce: which = 1 and 2 */
    const double* dinv;           /* kind "jacobi": init, update_xr: n values */
    SpmvAmdGcrMultiColumn* cols;  /* every vector stage but init: in; reduce: in and out -- k records, DEVICE memory */
    SpmvAmdPcgMultiColumn* shadow; /* reduce: out, `done` of each of the k records follows the column's -- DEVICE memory */
    double* partials;             /* the vector stages: out, value v of column j and workgroup g at [(v * k + j) * count + g] (multidot:
                                     `slot` values; orthogonalise: two; else one); reduce: in, the same layout */
    long long count;              /* the vector stages: out, the workgroups of the launch = (n + 255) / 256; reduce: in */
    int which;                    /* reduce: the scalar step, 0 = r0.r0, 1 = the betas of `slot`, 2 = gamma and rho, 3 = r.r */
    double tol;                   /* reduce, which = 3 */
    double* hist;                 /* reduce: k histories of hist_cap doubles one after the other (may be null when hist_cap is 0) */
    int hist_cap;
} SpmvAmdGcrMultiStageArgs;

/* The batched GCR solver's own kernels (csrc/gcr_multi.hip), one stage per call on the caller's device data -- the launches
 * spmv_amd_gcr_solve_device_multi makes, through the functions it makes them with, for k = 1..8 columns. The models are
 * spmv_amd_gcr_stage and spmv_amd_bicgstab_multi_stage; tests/test_gcr_multi_stages_gpu.py holds each stage against numpy. Every call
 * synchronises. kind: "none" or "jacobi" (init and update_xr; the others do not look at it). A column is RUNNING when cols[j].done
 * is 0. stage:
 *   "init"           R = fma(1.0, R, -1.0 * AX), "jacobi": ZS = dinv R, the partials of r.r; sets a->count
 *   "multidot"       for the running columns the partials of Q[i].Q[slot], i < slot, as value i (0.0 for the others); sets a->count
 *   "orthogonalise"  for the running columns, i ascending below slot: Q[slot] = fma(-beta_i, Q[i], Q[slot]) in place and z =
 *                    fma(-beta_i, Z[i], z) from z_in into Z[slot] (slot 0: z only moves), the partials of q.q (value 0) and r.q
 *                    (value 1); sets a->count
 *   "update_xr"      for the running columns x = fma(alpha, Z[slot], x), r = fma(-alpha, Q[slot], r), "jacobi": ZS = dinv r, the
 *                    partials of r.r; sets a->count
 *   "reduce"         the sums of a->count partials of the step's values per column, then the scalar step `which` on cols and shadow
 * A vector stage but init does nothing at all once every column is done, changes no bit of a column that is done, also where it shares
 * a 16-byte pair with a running one, and does not read a unit (one or two neighbouring columns of a row) without a running column.
 * Refused before any HIP call, with a sentence on stderr and a non-zero return: an unknown stage or kind, k outside 1..8, null
 * arguments, n < 1, count < 1, which outside 0..3, a slot outside the stage's range, hist_cap < 0, a null pointer the stage needs, a
 * block vector that is not 16-byte aligned, dinv, cols, shadow, partials or hist that are not 8-byte aligned. Returns 0 otherwise. */
int spmv_amd_gcr_multi_stage(const char* stage, const char* kind, int k, SpmvAmdGcrMultiStageArgs* a);

/* Device pointers of one spmv_amd_mg_multi_stage call; n = the FINE grid, the coarse grid is (n + 1) / 2. Block vectors are
 * row-interleaved, k columns: element (row, column j) at [row * k + j]. */
typedef struct SpmvAmdMgMultiStageArgs {
    int n;
    const int* row_ptr;      /* residual_restrict: the fine level's CSR, a complete 5-point stencil of grid n (checked) */
    const int* col_idx;
    const double* values;
    double* z;               /* residual_restrict: in; prolong: in and out; term0: out -- n * n rows */
    const double* r;         /* residual_restrict, term0: in -- n * n rows */
    double* coarse;          /* residual_restrict: out, r_c; prolong: in, e_c -- ((n + 1) / 2)^2 rows */
    double* d;               /* term0: out -- n * n rows */
    const double* dinv;      /* term0: n * n values */
    double c0;               /* term0 */
    const SpmvAmdPcgMultiColumn* cols; /* k records, DEVICE memory; null = every column is running. A launch does nothing at all
                                          when no record has done == 0 */
} SpmvAmdMgMultiStageArgs;
/* The batched multigrid cycle's own launches (csrc/multigrid_multi.hip), one per call on the caller's device data
 * for k = 1..8 columns, through the functions the cycle makes them with. Every call synchronises. stage: "residual_restrict"
 * (r_c = P^T (r - A z) per column in one launch), "prolong" (z = fma(2.0, e_c[agg(i)], z)), "term0" (d = c0 * (dinv * r); z = d).
 * Refused before any HIP call, with a [PCG-MULTI] sentence and a non-zero return: an unknown stage, k outside 1..8, null arguments,
 * n outside 2..46340, a null pointer the stage needs, a block vector that is not 16-byte (even k) or 8-byte (odd k) aligned, a CSR
 * array, dinv or cols that are not 4- / 8-byte aligned; after the structure check (as spmv_amd_mg_stage makes it): a CSR that is not the
 * complete stencil. Returns 0 otherwise. */
int spmv_amd_mg_multi_stage(const char* stage, int k, SpmvAmdMgMultiStageArgs* a);
/* The two launches a 3-D level adds to the batched cycle (csrc/multigrid3d_multi.hip; the checks are one body with
 * spmv_amd_mg_multi_stage's, in csrc/multigrid_multi.hip), on the same arguments: n is
 * the fine grid of n^3 rows, row_ptr / col_idx / values a complete 7-point stencil of it, coarse has ((n + 1) / 2)^3 rows. stage:
 * "residual_restrict3d", "prolong3d" (term 0 has no 3-D form: "term0" of spmv_amd_mg_multi_stage is a flat walk over the rows); and a
 * 3-D level's block product d = A z on the same CSR in its two kinds, "stencil7_spmm" ("spmm/stencil7-row-lds", csrc/stencil7_spmm.hip)
 * and "spmm_csr" ("spmm/csr"): z in, d out, n^3 rows each, the column records are not read. The checks are spmv_amd_mg_multi_stage's
 * with n in 2..674, all before any HIP call with a [PCG-MULTI] sentence, and the 7-point structure check as spmv_amd_mg_stage makes it
 * for its 3d stages behind them. Returns 0 otherwise. */
int spmv_amd_mg_multi_stage3d(const char* stage, int k, SpmvAmdMgMultiStageArgs* a);
/* The block product the levels of the 3-D hierarchies made AFTER this call get (spmv_amd_precond_create_multigrid3d_multi): "auto" (the
 * default: "spmm/stencil7-row-lds" from the threshold grid upward, "spmm/csr" below it), "csr" or "stencil7" on every level. Read when a
 * hierarchy is made, never on a launch path. Non-zero, with a [PCG-MULTI] sentence, for any other word. */
int spmv_amd_mg3d_multi_level_product(const char* kind);
/* The name of one level's SpMM plan in a hierarchy with block vectors ("spmm/csr", "spmm/stencil7-row-lds", "spmm/stencil5-row-lds",
 * ...); "none" for NULL, another kind, a single-vector hierarchy or a level that does not exist. */
const char* spmv_amd_precond_multigrid_level_spmm(const SpmvAmdPrecond* m, int level);

/* One fused launch of an operator of this library, as cg_solve_device puts it into its loop (csrc/operators.hip, fused_spmv_of), on
 * the caller's DEVICE vectors: d_y = A d_x and, in d_partials, the launch's partials of x . (A x), unreduced -- one per logical block
 * of the CSR stream / adaptive kernels, per 256 rows of the ELLPACK kernels, per tile of the stencil kernels. Synchronises; *count
 * (host) = the number of partials written. Refused before any HIP call, with a [fused-spmv] sentence on stderr and a non-zero return:
 * null arguments, a table this library does not own, an operator used before init, an operator with no fused form (csr/row-scalar,
 * csr/wavefront, a rectangular matrix: their loop runs run_device, then a dot pass) and cap below the number of partials. Returns 0
 * otherwise. */
int spmv_amd_operator_fused_spmv(const SpmvOperator* op, const double* d_x, double* d_y, double* d_partials, int cap, int* count);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_AMD_LAB_H */
