// operators.hip -- the SpmvOperator tables behind get_operator().
//
//   "stencil5-csr"     <- reference SPMV_STENCIL5_CSR, src/spmv/spmv_stencil_csr_direct.cu:194-307
//   "cusparse-csr"     <- reference SPMV_CSR, src/spmv/spmv_cusparse_csr.cu:182-327 (the cuSPARSE
//                         call is replaced by this build's own CSR kernels; the name is kept so that
//                         calculate_spmv_metrics and the harness scripts keep working)
//   "stencil7-csr"     <- no reference counterpart: the n x n x n 7-point stencil (stencil7_kernels.hip)
//   "ellpack",
//   "stencil5-ellpack" <- reference include/spmv_ellpack.h, include/spmv_stencil.h:25-42 (headers only)
//
// Lifecycle, ownership and error behaviour follow the reference: init builds the host CSR
// through build_csr_struct (kept in csr_mat for the other operators), uploads it, and allocates
// the x/y staging vectors; run_timed copies x in, times the kernel alone with events, copies y
// out; run_device enqueues on the default stream and returns; free drops device memory only.
// One live instance per operator per process (file-static state, as upstream).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "device_runtime.hpp"
#include "multi_rhs.hpp"
#include "stencil_geometry.hpp"
#ifdef SPMV_AMD_LAB
#include "spmv_amd/lab.h"
#endif

using namespace spmv_amd;

namespace {

constexpr hipStream_t kDefaultStream = nullptr;  // the reference launches on the default stream

struct CsrBackedOperator {
    const char* tag;
    LaunchShape shape;        // the launch switches (kernels.hpp), read when a variant is picked
    Stencil5Plan plan;        // stencil5-csr: the launch plan of the whole matrix, made once per init / variant change
    DeviceCsr A;
    double* dX = nullptr;
    double* dY = nullptr;
    int rows = 0, cols = 0;
    bool ready = false;
    Stencil5Variant stencil_variant = Stencil5Variant::Auto;
    CsrVariant csr_variant = CsrVariant::Auto;
    const char* variant_name = "uninitialised";
    // stencil7-csr: the 3-D geometry lives here, not in the view (whose grid_size / verified_stencil mean "2-D 5-point")
    Stencil7Plan plan7;
    Stencil7Variant stencil7_variant = Stencil7Variant::Auto;
    int grid7 = 0;             // n of the verified n^3 grid, 0 otherwise
    bool verified7 = false;

    int tuned_run = 0;         // stencil5-csr: row-lds tiles per XCD and run kept by the set-up trial (0 = not tried yet, -1 = does not apply)
    double tuning[4] = {0, 0, 0, 0};  // {rule, kept, ms with the rule, ms kept}
    int y_candidates = 1;      // output placement: candidates timed for dY, and what the choice was worth (device_runtime.hpp)
    double y_gain = 1.0;
    unsigned long long generation = 0;  // bumped by every init and free (drop()): what a preconditioner was made from (precond.hip)
    void alloc_vectors() {
        dX = device_alloc<double>((size_t)cols);
        dY = nullptr;  // placed by place_output() once the kernel that writes it is known
    }
    // dY = the fastest of a few allocations for THIS operator's kernel reading dX (ones) and writing the candidate: the vector
    // run_timed's kernel writes (reference harness: main.cu:158-187 times run_timed). Vectors under 16 M rows are taken as they come.
    template <class Launch>
    void place_output(Launch&& launch) {
        device_release(dY);
        launch_fill(dX, (size_t)cols, 1.0, kDefaultStream);
        EventTimer t;
        dY = device_alloc_best_of<double>((size_t)rows, (size_t)16 << 20, [&](double* y) {
            float ms[3];
            launch(dX, y);
            for (float& m : ms) {
                t.begin(kDefaultStream);
                launch(dX, y);
                t.end(kDefaultStream);
                m = t.elapsed_ms();
            }
            std::sort(ms, ms + 3);
            return (double)ms[1];
        }, &y_candidates, &y_gain);
        HIP_CHECK(hipStreamSynchronize(kDefaultStream));
    }
    int init_from_host(MatrixData* mat, bool grid_in_view = true) {
        if (build_csr_struct(mat) != EXIT_SUCCESS) return EXIT_FAILURE;
        drop();
        rows = csr_mat.nb_rows;
        cols = csr_mat.nb_cols;
        A.upload_slab(csr_mat, 0, rows, grid_in_view ? mat->grid_size : -1);
        A.view.halo_after = cols - rows;  // x is readable on [0, cols)
        alloc_vectors();
        ready = true;
        return 0;
    }
    int init_synthetic(int n) {
        drop();
        if (n < 1 || (long long)n * n > 0x7fffffffLL || 5LL * n * n - 4LL * n > 0x7fffffffLL) {
            fprintf(stderr, "[%s] grid %d does not fit 32-bit CSR indices\n", tag, n);
            return EXIT_FAILURE;
        }
        rows = cols = n * n;
        A.generate_stencil5(n, 0, rows, 5.0, -1.0, kDefaultStream);
        // dimensions for calculate_spmv_metrics; the host arrays do not exist on this path
        spmv_amd_reset_host_matrices();
        csr_mat.nb_rows = rows;
        csr_mat.nb_cols = cols;
        csr_mat.nb_nonzeros = (int)A.view.nnz_local;
        alloc_vectors();
        ready = true;
        return 0;
    }
    // the n^3 generator matrix (centre 7, neighbours -1 unless told otherwise) built in HBM; the caller has checked stencil7_fits_int32(n)
    int init_synthetic7(int n, double center = 7.0, double off = -1.0) {
        drop();
        rows = cols = n * n * n;
        A.generate_stencil7(n, center, off, kDefaultStream);
        spmv_amd_reset_host_matrices();
        csr_mat.nb_rows = rows;
        csr_mat.nb_cols = cols;
        csr_mat.nb_nonzeros = (int)A.view.nnz_local;
        alloc_vectors();
        ready = true;
        return 0;
    }
    void drop() {
        grid7 = 0;
        verified7 = false;
        A.release();
        device_release(dX);
        device_release(dY);
        ++generation;
        ready = false;
        tuned_run = 0;
        variant_name = "uninitialised";
    }
};

CsrBackedOperator g_stencil{"stencil5-csr"};
CsrBackedOperator g_csr{"cusparse-csr"};
CsrBackedOperator g_stencil7{"stencil7-csr"};

// ---- stencil5-csr ----------------------------------------------------------------

void stencil_pick_variant() {
    g_stencil.shape = current_launch_shape();
    g_stencil.plan = plan_stencil5(g_stencil.A.view, 0, g_stencil.rows, g_stencil.stencil_variant, g_stencil.shape);
    g_stencil.variant_name = g_stencil.plan.name;
    if (g_stencil.dY == nullptr) {  // once per init: the class a good output vector lies in does not depend on the variant
        g_stencil.place_output([](const double* x, double* y) {
            (void)launch_stencil5_spmv(g_stencil.A.view, g_stencil.plan, x, y, 1.0, nullptr, nullptr, false, kDefaultStream);
        });
        g_stencil.tuned_run = 0;
    }
    // row-lds tiles per XCD and run: the rule's neighbours timed once per init on the operator's own vectors (device_runtime.hpp)
    if (g_stencil.stencil_variant == Stencil5Variant::Auto || g_stencil.stencil_variant == Stencil5Variant::RowLds) {
        if (g_stencil.tuned_run == 0 && g_stencil.shape.knobs.rowlds_group == 0) {
            const int run = tune_rowlds_xcd_run(g_stencil.A.view, g_stencil.shape, g_stencil.dX, g_stencil.dY, nullptr, kDefaultStream, g_stencil.tuning);
            g_stencil.tuned_run = run > 0 ? run : -1;
        }
        if (g_stencil.tuned_run > 0 && g_stencil.shape.knobs.rowlds_group == 0) {
            g_stencil.shape.knobs.rowlds_group = g_stencil.tuned_run;
            g_stencil.plan = plan_stencil5(g_stencil.A.view, 0, g_stencil.rows, g_stencil.stencil_variant, g_stencil.shape);
        }
    }
}

int stencil_init(MatrixData* mat) {
    printf("[stencil5-csr] Initializing (computed offsets, row-lds / row-direct kernels on gfx950)\n");
    if (g_stencil.init_from_host(mat) != 0) return EXIT_FAILURE;
    g_stencil.A.verify_stencil(kDefaultStream);
    stencil_pick_variant();
    printf("[stencil5-csr] %d rows, %d nnz, grid %dx%d, variant %s\n", csr_mat.nb_rows,
           csr_mat.nb_nonzeros, mat->grid_size, mat->grid_size, g_stencil.variant_name);
    if (g_stencil.tuned_run > 0)
        printf("[stencil5-csr] tiles per XCD and run: %d kept (rule %d: %.4f ms, kept %.4f ms)\n", g_stencil.tuned_run, (int)g_stencil.tuning[0],
               g_stencil.tuning[2], g_stencil.tuning[3]);
    return 0;
}

int stencil_run_device(const double* d_x, double* d_y) {
    if (!g_stencil.ready) {
        fprintf(stderr, "[stencil5-csr] run before init\n");
        return EXIT_FAILURE;
    }
    (void)launch_stencil5_spmv(g_stencil.A.view, g_stencil.plan, d_x, d_y, /*alpha=*/1.0, nullptr, nullptr,
                               /*reverse=*/false, kDefaultStream);
    return 0;
}

template <int (*RunDevice)(const double*, double*), CsrBackedOperator* Op>
int run_timed_generic(const double* x, double* y, double* kernel_time_ms) {
    if (!Op->ready) {
        fprintf(stderr, "[%s] run before init\n", Op->tag);
        return EXIT_FAILURE;
    }
    upload(Op->dX, x, (size_t)Op->cols);
    EventTimer t;
    t.begin(kDefaultStream);
    RunDevice(Op->dX, Op->dY);
    t.end(kDefaultStream);
    *kernel_time_ms = (double)t.elapsed_ms();
    HIP_CHECK(hipGetLastError());
    download(y, Op->dY, (size_t)Op->rows);
    return 0;
}

void stencil_free() {
    printf("[stencil5-csr] Cleaning up\n");
    release_cg_workspace();  // the single-GPU CG solver's vectors live as long as an operator does
    g_stencil.drop();
}

// The launch cg_solve_device uses when the operator it is handed is this one (device_runtime.hpp, FusedSpmv).
int stencil_fused_launch(const double* d_x, double* d_y, double* d_partials, const int* d_skip, bool reverse,
                         const ResidualOut* init, hipStream_t stream) {
    return launch_stencil5_spmv(g_stencil.A.view, g_stencil.plan, d_x, d_y, /*alpha=*/1.0, d_partials, d_skip, reverse, stream, init);
}

// ---- stencil7-csr ----------------------------------------------------------------
// A matrix is the 3-D operator's own when grid_size = n >= 2, rows == cols == n^3, nnz == 7 n^3 - 6 n^2 and every row has the
// complete pattern; anything else runs every row through the CSR launcher ("stencil7/csr-loop").
void stencil7_verify(int n) {
    CsrBackedOperator& o = g_stencil7;
    o.grid7 = 0;
    o.verified7 = false;
    // the sizes first: the verifier's analytic offsets must not run past the arrays
    if (n < 2 || !stencil7_fits_int32(n) || o.rows != o.cols || (long long)n * n * n != o.rows || o.A.view.nnz_local != stencil7_nnz(n)) return;
    int* d_flag = device_alloc<int>(1);
    HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), kDefaultStream));
    launch_verify_stencil7_csr(o.A.view, n, d_flag, kDefaultStream);
    int h_flag = 1;
    HIP_CHECK(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, kDefaultStream));
    HIP_CHECK(hipStreamSynchronize(kDefaultStream));
    device_release(d_flag);
    o.verified7 = h_flag == 0;
    if (o.verified7) o.grid7 = n;
}

void stencil7_pick_variant() {
    CsrBackedOperator& o = g_stencil7;
    o.shape = current_launch_shape();
    o.plan7 = plan_stencil7(o.A.view, o.grid7, o.verified7, o.stencil7_variant, o.shape.knobs);
    o.variant_name = o.plan7.name;
    if (o.dY == nullptr)  // once per init, as for the other operators
        o.place_output([](const double* x, double* y) {
            (void)launch_stencil7_spmv(g_stencil7.A.view, g_stencil7.plan7, x, y, 1.0, nullptr, nullptr, false, kDefaultStream);
        });
}

int stencil7_init(MatrixData* mat) {
    printf("[stencil7-csr] Initializing (7-point stencil of an n^3 grid: row-lds / row-direct kernels on gfx950)\n");
    if (g_stencil7.init_from_host(mat, /*grid_in_view=*/false) != 0) return EXIT_FAILURE;
    stencil7_verify(mat->grid_size);
    stencil7_pick_variant();
    printf("[stencil7-csr] %d rows, %d nnz, grid %d^3, variant %s\n", csr_mat.nb_rows, csr_mat.nb_nonzeros, g_stencil7.grid7,
           g_stencil7.variant_name);
    return 0;
}

int stencil7_run_device(const double* d_x, double* d_y) {
    if (!g_stencil7.ready) {
        fprintf(stderr, "[stencil7-csr] run before init\n");
        return EXIT_FAILURE;
    }
    (void)launch_stencil7_spmv(g_stencil7.A.view, g_stencil7.plan7, d_x, d_y, /*alpha=*/1.0, nullptr, nullptr, /*reverse=*/false, kDefaultStream);
    return 0;
}

void stencil7_free() {
    printf("[stencil7-csr] Cleaning up\n");
    release_cg_workspace();
    g_stencil7.drop();
}

// cg_solve_device's fused launch: p . Ap partials from inside the SpMV; no fused initial residual (the loop streams it)
int stencil7_fused_launch(const double* d_x, double* d_y, double* d_partials, const int* d_skip, bool reverse, const ResidualOut* init,
                          hipStream_t stream) {
    if (init != nullptr) return -1;
    return launch_stencil7_spmv(g_stencil7.A.view, g_stencil7.plan7, d_x, d_y, /*alpha=*/1.0, d_partials, d_skip, reverse, stream);
}

// ---- cusparse-csr ----------------------------------------------------------------

const char* csr_variant_name(CsrVariant v, const SlabCsr& m) {
    if (v == CsrVariant::Auto) v = csr_auto_variant(m);
    switch (v) {
        case CsrVariant::Stream: return "csr/stream";
        case CsrVariant::Adaptive: return "csr/adaptive";
        case CsrVariant::RowScalar: return "csr/row-scalar";
        default: return "csr/wavefront";
    }
}

void csr_place_output();

int csr_init(MatrixData* mat) {
    if (g_csr.init_from_host(mat) != 0) return EXIT_FAILURE;
    g_csr.variant_name = csr_variant_name(g_csr.csr_variant, g_csr.A.view);
    csr_place_output();
    printf("[cusparse-csr] %d rows, %d nnz, variant %s\n", csr_mat.nb_rows, csr_mat.nb_nonzeros,
           g_csr.variant_name);
    return EXIT_SUCCESS;
}

void csr_place_output() {
    if (g_csr.dY == nullptr)
        g_csr.place_output([](const double* x, double* y) {
            launch_csr_spmv(g_csr.A.view, x, y, 1.0, g_csr.csr_variant, kDefaultStream);
        });
}

int csr_run_device(const double* d_x, double* d_y) {
    if (!g_csr.ready) {
        fprintf(stderr, "[cusparse-csr] run before init\n");
        return EXIT_FAILURE;
    }
    launch_csr_spmv(g_csr.A.view, d_x, d_y, /*alpha=*/1.0, g_csr.csr_variant, kDefaultStream);
    return EXIT_SUCCESS;
}

// cg_solve_device's fused launches for the operators other than stencil5-csr: the SpMV kernel also writes the partial sums of
// x . (A x) (one per workgroup), so the loop needs no 16 B/row dot pass. No skip flag (the loop never enqueues a SpMV past
// convergence), no sweep direction, no fused initial residual.
int csr_fused_launch(const double* d_x, double* d_y, double* d_partials, const int*, bool, const ResidualOut* init, hipStream_t stream) {
    if (init != nullptr) return -1;
    launch_csr_spmv(g_csr.A.view, d_x, d_y, /*alpha=*/1.0, g_csr.csr_variant, stream, d_partials);
    return csr_fused_dot_partials(g_csr.A.view, g_csr.csr_variant);
}

void csr_free() {
    printf("[CSR] Cleaning up\n");
    release_cg_workspace();
    g_csr.drop();
}

// ---- ellpack / stencil5-ellpack -----------------------------------------------------

struct EllOperator {
    const char* tag;
    bool stencil_fast_path;
    // slot-major planes, both carved out of ONE allocation (val first): the kernel reads val[k][r] and idx[k][r] in lock step
    // (DeviceCsr::allocate has the reason)
    char* planes_block = nullptr;
    int* idx = nullptr;
    double* val = nullptr;
    void alloc_planes(size_t slots) {
        const size_t v_bytes = (slots * sizeof(double) + 4095) / 4096 * 4096;
        planes_block = device_alloc<char>(v_bytes + slots * sizeof(int));
        val = reinterpret_cast<double*>(planes_block);
        idx = reinterpret_cast<int*>(planes_block + v_bytes);
    }
    double* dX = nullptr;
    double* dY = nullptr;
    int rows = 0, cols = 0, width = 0, grid_size = -1;
    bool verified = false;
    bool ready = false;
    const char* variant_name = "uninitialised";
    int y_candidates = 1;  // output placement (device_runtime.hpp)
    double y_gain = 1.0;
    unsigned long long generation = 0;  // as CsrBackedOperator's
    void drop() {
        ++generation;
        device_release(planes_block);
        idx = nullptr;
        val = nullptr;
        device_release(dX);
        device_release(dY);
        ready = false;
        variant_name = "uninitialised";
    }
    void pick() {
        variant_name = (stencil_fast_path && verified && grid_size >= 3) ? "ell/stencil5-direct"
                                                                        : "ell/slot-major";
    }
};

EllOperator g_ell{"ellpack", false};
EllOperator g_ell_stencil{"stencil5-ellpack", true};

__global__ void csr_to_ell_slotmajor_kernel(SlabCsr m, int width, int* __restrict__ idx,
                                            double* __restrict__ val) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_local) return;
    const int lo = m.row_ptr[r], len = m.row_ptr[r + 1] - lo;
    for (int k = 0; k < width; ++k) {
        const bool live = k < len;
        idx[(long long)k * m.n_local + r] = live ? m.col_idx[lo + k] : -1;
        val[(long long)k * m.n_local + r] = live ? m.values[lo + k] : 0.0;
    }
}

int ell_run(EllOperator& op, const double* d_x, double* d_y, double alpha, double beta);

// the vector the operator's kernel writes: the fastest of a few allocations (device_runtime.hpp, output placement)
void ell_place_output(EllOperator& op) {
    launch_fill(op.dX, (size_t)op.cols, 1.0, kDefaultStream);
    EventTimer t;
    op.dY = device_alloc_best_of<double>((size_t)op.rows, (size_t)16 << 20, [&](double* y) {
        float ms[3];
        ell_run(op, op.dX, y, 1.0, 0.0);
        for (float& m : ms) {
            t.begin(kDefaultStream);
            ell_run(op, op.dX, y, 1.0, 0.0);
            t.end(kDefaultStream);
            m = t.elapsed_ms();
        }
        std::sort(ms, ms + 3);
        return (double)ms[1];
    }, &op.y_candidates, &op.y_gain);
    HIP_CHECK(hipStreamSynchronize(kDefaultStream));
}

int ell_init_common(EllOperator& op, MatrixData* mat) {
    if (ensure_ellpack_structure_built(mat) != EXIT_SUCCESS) return EXIT_FAILURE;
    op.drop();
    const ELLPACKMatrix& E = ellpack_matrix;
    op.rows = E.nb_rows, op.cols = E.nb_cols, op.width = E.ell_width, op.grid_size = mat->grid_size;
    const size_t slots = (size_t)op.rows * op.width;
    int* idx_rm = device_alloc<int>(slots);
    double* val_rm = device_alloc<double>(slots);
    upload(idx_rm, E.indices, slots);
    upload(val_rm, E.values, slots);
    op.alloc_planes(slots);
    launch_ell_transpose(op.rows, op.width, idx_rm, val_rm, op.idx, op.val, kDefaultStream);
    HIP_CHECK(hipStreamSynchronize(kDefaultStream));
    device_release(idx_rm);
    device_release(val_rm);
    op.verified = false;
    if (op.stencil_fast_path && csr_mat.row_ptr != nullptr) {
        DeviceCsr probe;  // structure check on the CSR the ELL was built from
        probe.upload_slab(csr_mat, 0, op.rows, mat->grid_size);
        probe.verify_stencil(kDefaultStream);
        op.verified = probe.view.verified_stencil;
        probe.release();
    }
    op.dX = device_alloc<double>((size_t)op.cols);
    op.ready = true;
    op.pick();
    ell_place_output(op);
    printf("[%s] %d rows, width %d, variant %s\n", op.tag, op.rows, op.width, op.variant_name);
    return 0;
}

int ell_init_synthetic(EllOperator& op, int n) {
    op.drop();
    DeviceCsr src;
    if ((long long)n * n > 0x7fffffffLL || 5LL * n * n > 0x7fffffffLL) return EXIT_FAILURE;
    src.generate_stencil5(n, 0, n * n, 5.0, -1.0, kDefaultStream);
    op.rows = op.cols = n * n;
    op.width = n >= 3 ? 5 : (n == 2 ? 3 : 1);
    op.grid_size = n;
    const size_t slots = (size_t)op.rows * op.width;
    op.alloc_planes(slots);
    hipLaunchKernelGGL(csr_to_ell_slotmajor_kernel, dim3((op.rows + 255) / 256), dim3(256), 0,
                       kDefaultStream, src.view, op.width, op.idx, op.val);
    HIP_CHECK(hipStreamSynchronize(kDefaultStream));
    src.release();
    op.verified = true;
    spmv_amd_reset_host_matrices();
    csr_mat.nb_rows = csr_mat.nb_cols = op.rows;
    csr_mat.nb_nonzeros = (int)(5LL * n * n - 4LL * n);
    op.dX = device_alloc<double>((size_t)op.cols);
    op.ready = true;
    op.pick();
    ell_place_output(op);
    return 0;
}

int ell_run(EllOperator& op, const double* d_x, double* d_y, double alpha = 1.0, double beta = 0.0);
int ell_run(EllOperator& op, const double* d_x, double* d_y, double alpha, double beta) {
    if (!op.ready) {
        fprintf(stderr, "[%s] run before init\n", op.tag);
        return EXIT_FAILURE;
    }
    if (op.stencil_fast_path && op.verified)
        launch_ell_stencil5_spmv(op.rows, op.width, op.grid_size, op.idx, op.val, d_x, d_y, alpha, beta, kDefaultStream);
    else
        launch_ell_spmv(op.rows, op.width, op.idx, op.val, d_x, d_y, alpha, beta, kDefaultStream, op.verified ? op.grid_size : 0);
    return 0;
}

int ell_run_timed(EllOperator& op, const double* x, double* y, double* kernel_time_ms) {
    if (!op.ready) return EXIT_FAILURE;
    upload(op.dX, x, (size_t)op.cols);
    EventTimer t;
    t.begin(kDefaultStream);
    ell_run(op, op.dX, op.dY);
    t.end(kDefaultStream);
    *kernel_time_ms = (double)t.elapsed_ms();
    HIP_CHECK(hipGetLastError());
    download(y, op.dY, (size_t)op.rows);
    return 0;
}

template <EllOperator* Op>
int ell_fused_launch(const double* d_x, double* d_y, double* d_partials, const int*, bool, const ResidualOut* init, hipStream_t stream) {
    if (init != nullptr || !Op->ready) return -1;
    if (Op->stencil_fast_path && Op->verified)
        launch_ell_stencil5_spmv(Op->rows, Op->width, Op->grid_size, Op->idx, Op->val, d_x, d_y, 1.0, 0.0, stream, d_partials);
    else
        launch_ell_spmv(Op->rows, Op->width, Op->idx, Op->val, d_x, d_y, 1.0, 0.0, stream, Op->verified ? Op->grid_size : 0, d_partials);
    return ell_fused_dot_partials(Op->rows);
}

int ellg_init(MatrixData* m) { return ell_init_common(g_ell, m); }
int ellg_run_timed(const double* x, double* y, double* ms) { return ell_run_timed(g_ell, x, y, ms); }
int ellg_run_device(const double* x, double* y) { return ell_run(g_ell, x, y); }
void ellg_free() {
    release_cg_workspace();
    g_ell.drop();
}
int ells_init(MatrixData* m) { return ell_init_common(g_ell_stencil, m); }
int ells_run_timed(const double* x, double* y, double* ms) { return ell_run_timed(g_ell_stencil, x, y, ms); }
int ells_run_device(const double* x, double* y) { return ell_run(g_ell_stencil, x, y); }
void ells_free() {
    release_cg_workspace();
    g_ell_stencil.drop();
}

// ---- name table ------------------------------------------------------------------

enum class Which { None, Stencil, Csr, Ell, EllStencil, Stencil7 };

Which which_operator(const char* mode) {
    if (!mode) return Which::None;
    if (!strcmp(mode, "stencil5-csr") || !strcmp(mode, "stencil5")) return Which::Stencil;
    if (!strcmp(mode, "stencil7-csr") || !strcmp(mode, "stencil7")) return Which::Stencil7;
    if (!strcmp(mode, "cusparse-csr") || !strcmp(mode, "csr")) return Which::Csr;
    if (!strcmp(mode, "ellpack")) return Which::Ell;
    if (!strcmp(mode, "stencil5-ellpack")) return Which::EllStencil;
    return Which::None;
}

}  // namespace

SpmvOperator SPMV_STENCIL5_CSR = {"stencil5-csr", stencil_init,
                                  run_timed_generic<stencil_run_device, &g_stencil>,
                                  stencil_run_device, stencil_free};
SpmvOperator SPMV_CSR = {"cusparse-csr", csr_init, run_timed_generic<csr_run_device, &g_csr>,
                         csr_run_device, csr_free};
SpmvOperator SPMV_STENCIL7_CSR = {"stencil7-csr", stencil7_init, run_timed_generic<stencil7_run_device, &g_stencil7>,
                                  stencil7_run_device, stencil7_free};
SpmvOperator SPMV_ELLPACK = {"ellpack", ellg_init, ellg_run_timed, ellg_run_device, ellg_free};
SpmvOperator SPMV_STENCIL5_ELLPACK = {"stencil5-ellpack", ells_init, ells_run_timed,
                                      ells_run_device, ells_free};
// Upstream declares this table under __has_include(<mpi.h>) and never defines it; here the
// multi-GPU SpMV lives in the slab solver (cg_slab.hip), so the name resolves to the
// single-GPU stencil operator.
SpmvOperator SPMV_STENCIL_HALO_MGPU = {"stencil5-halo-mgpu", stencil_init,
                                       run_timed_generic<stencil_run_device, &g_stencil>,
                                       stencil_run_device, stencil_free};

namespace {
// Which of this library's operators `op` is: its CSR-backed state, its ELLPACK state, or neither (a table this library does
// not own). "stencil5-halo-mgpu" is the stencil operator under another name. Host state only (no HIP call).
struct OwnOperator {
    CsrBackedOperator* csr = nullptr;
    EllOperator* ell = nullptr;
};
OwnOperator own_operator_of(const SpmvOperator* op) {
    OwnOperator o;
    if (op == &SPMV_STENCIL5_CSR || op == &SPMV_STENCIL_HALO_MGPU) o.csr = &g_stencil;
    else if (op == &SPMV_CSR) o.csr = &g_csr;
    else if (op == &SPMV_STENCIL7_CSR) o.csr = &g_stencil7;
    else if (op == &SPMV_ELLPACK) o.ell = &g_ell;
    else if (op == &SPMV_STENCIL5_ELLPACK) o.ell = &g_ell_stencil;
    return o;
}
}  // namespace

namespace spmv_amd {
FusedSpmv fused_spmv_of(const SpmvOperator* op) {
    FusedSpmv f;
    const OwnOperator o = own_operator_of(op);
    // (the row-generic kernel of small or unverified matrices keeps the plain dot kernel, as in the slab solver)
    if (o.csr == &g_stencil && g_stencil.ready && g_stencil.plan.partials > 0 && g_stencil.plan.variant != Stencil5Variant::RowGeneric) {
        f.partials = g_stencil.plan.partials;
        f.can_init = g_stencil.plan.variant == Stencil5Variant::RowLds;
        f.launch = stencil_fused_launch;
    } else if (o.csr == &g_stencil7 && g_stencil7.ready && g_stencil7.rows == g_stencil7.cols) {
        // row-lds / row-direct: the kernels' own partials; csr-loop: what cusparse-csr has (0 = run_device, then a dot pass)
        f.partials = g_stencil7.plan7.partials;
        f.launch = f.partials > 0 ? stencil7_fused_launch : nullptr;
    } else if (o.csr == &g_csr && g_csr.ready && g_csr.rows == g_csr.cols) {
        f.partials = csr_fused_dot_partials(g_csr.A.view, g_csr.csr_variant);
        f.launch = f.partials > 0 ? csr_fused_launch : nullptr;
    } else if (o.ell != nullptr && o.ell->ready && o.ell->rows == o.ell->cols) {
        f.partials = ell_fused_dot_partials(o.ell->rows);
        f.launch = o.ell == &g_ell ? ell_fused_launch<&g_ell> : ell_fused_launch<&g_ell_stencil>;
    }
    return f;
}
}  // namespace spmv_amd

#ifdef SPMV_AMD_LAB
// (LAB build only; include/spmv_amd/lab.h.) One fused launch of an operator -- the SpMV cg_solve_device puts into its loop -- on the
// caller's device vectors: y = A x and the launch's partials of x . (A x), unreduced. Every refusal comes before any HIP call.
extern "C" int spmv_amd_operator_fused_spmv(const SpmvOperator* op, const double* d_x, double* d_y, double* d_partials, int cap, int* count) {
    auto refuse = [](const char* why) {
        fprintf(stderr, "[fused-spmv] refused: %s\n", why);
        return EXIT_FAILURE;
    };
    if (op == nullptr || d_x == nullptr || d_y == nullptr || d_partials == nullptr || count == nullptr) return refuse("null arguments");
    const OwnOperator o = own_operator_of(op);
    if (o.csr == nullptr && o.ell == nullptr) return refuse("the operator is not one of this library's tables");
    if (!(o.csr != nullptr ? o.csr->ready : o.ell->ready)) return refuse("the operator is used before init");
    const FusedSpmv f = fused_spmv_of(op);
    if (f.partials <= 0 || f.launch == nullptr) return refuse("the operator has no fused form (its loop runs run_device, then a dot pass)");
    if (cap < f.partials) return refuse("cap is below the number of partials the launch writes");
    const int used = f.launch(d_x, d_y, d_partials, nullptr, false, nullptr, kDefaultStream);
    HIP_CHECK(hipStreamSynchronize(kDefaultStream));
    HIP_CHECK(hipGetLastError());
    *count = used;
    return used > 0 ? 0 : EXIT_FAILURE;
}
#endif  // SPMV_AMD_LAB

namespace spmv_amd {
ChebSpmv cheb_spmv_of(const SpmvOperator* op) {
    ChebSpmv c;
    c.op = op;
    if (own_operator_of(op).csr == &g_stencil && g_stencil.ready) {
        c.view = &g_stencil.A.view, c.plan = &g_stencil.plan;
        if (g_stencil.plan.variant == Stencil5Variant::RowLds) c.partials = g_stencil.plan.partials;
    }
    return c;
}

// The multi-RHS path (multi_rhs.hpp, spmm_kernels.hip): the stencil operator's SpMM follows its single-vector variant; the CSR
// operator's is the sequential thread-per-row kernel whatever its single-vector variant. The ELLPACK operators have none.
MultiOperand multi_operand_of(const SpmvOperator* op) {
    MultiOperand o;
    const CsrBackedOperator* c = own_operator_of(op).csr;
    if (c == nullptr) return o;
    o.has_multi = true;
    o.ready = c->ready;
    const bool stencil = c == &g_stencil;
    if (o.ready) o.plan = plan_spmm(c->A.view, stencil ? g_stencil.plan.variant : Stencil5Variant::Auto, !stencil, c->rows, c->cols);
    return o;
}

// Where a Jacobi preconditioner reads the diagonal (precond.hip): the operator's own device storage, no copy.
DiagonalSource diagonal_source_of(const SpmvOperator* op) {
    DiagonalSource d;
    const OwnOperator o = own_operator_of(op);
    const CsrBackedOperator* c = o.csr;
    const EllOperator* e = o.ell;
    if (c != nullptr) {
        d.owner = c;
        d.kind = DiagonalSource::Csr;
        d.ready = c->ready;
        d.rows = c->rows, d.cols = c->cols;
        d.generation = c->generation;
        d.csr = c->A.view;
    } else if (e != nullptr) {
        d.owner = e;
        d.kind = DiagonalSource::Ell;
        d.ready = e->ready;
        d.rows = e->rows, d.cols = e->cols;
        d.generation = e->generation;
        d.idx = e->idx, d.val = e->val, d.width = e->width;
    }
    return d;
}

Stencil7Source stencil7_source_of(const SpmvOperator* op) {
    Stencil7Source s;
    if (own_operator_of(op).csr == &g_stencil7 && g_stencil7.ready) {
        s.grid = g_stencil7.grid7, s.verified = g_stencil7.verified7;
        s.csr_loop = g_stencil7.plan7.variant == Stencil7Variant::CsrLoop;
        s.plan_name = g_stencil7.plan7.name;
    }
    return s;
}
}  // namespace spmv_amd

extern "C" SpmvOperator* get_operator(const char* mode) {
    switch (which_operator(mode)) {
        case Which::Stencil: return &SPMV_STENCIL5_CSR;
        case Which::Csr: return &SPMV_CSR;
        case Which::Stencil7: return &SPMV_STENCIL7_CSR;
        case Which::Ell: return &SPMV_ELLPACK;
        case Which::EllStencil: return &SPMV_STENCIL5_ELLPACK;
        default: break;
    }
    if (mode && !strcmp(mode, "stencil5-halo-mgpu")) return &SPMV_STENCIL_HALO_MGPU;
    return nullptr;
}

extern "C" int spmv_amd_init_stencil5_synthetic(const char* mode, int n) {
    switch (which_operator(mode)) {
        case Which::Stencil:
            if (g_stencil.init_synthetic(n) != 0) return EXIT_FAILURE;
            g_stencil.A.verify_stencil(kDefaultStream);
            stencil_pick_variant();
            return 0;
        case Which::Csr:
            if (g_csr.init_synthetic(n) != 0) return EXIT_FAILURE;
            HIP_CHECK(hipStreamSynchronize(kDefaultStream));
                    g_csr.variant_name = csr_variant_name(g_csr.csr_variant, g_csr.A.view);
            csr_place_output();
            return 0;
        case Which::Ell: return ell_init_synthetic(g_ell, n);
        case Which::EllStencil: return ell_init_synthetic(g_ell_stencil, n);
        default: return EXIT_FAILURE;
    }
}

extern "C" int spmv_amd_init_stencil7_synthetic(const char* mode, int n) { return spmv_amd_init_stencil7_synthetic_values(mode, n, 7.0, -1.0); }

extern "C" int spmv_amd_init_stencil7_synthetic_values(const char* mode, int n, double center, double off) {
    // rows = n^3 and nnz = 7 n^3 - 6 n^2 must fit int32 (n <= 674): decided before any HIP call
    if (!stencil7_fits_int32(n)) {
        fprintf(stderr, "[stencil7] grid %d^3 is refused: 1 <= n <= 674 keeps rows and nnz inside 32-bit CSR indices\n", n);
        return EXIT_FAILURE;
    }
    switch (which_operator(mode)) {
        case Which::Stencil7:
            if (g_stencil7.init_synthetic7(n, center, off) != 0) return EXIT_FAILURE;
            stencil7_verify(n);
            stencil7_pick_variant();
            return 0;
        case Which::Csr:
            if (g_csr.init_synthetic7(n, center, off) != 0) return EXIT_FAILURE;
            HIP_CHECK(hipStreamSynchronize(kDefaultStream));
            g_csr.variant_name = csr_variant_name(g_csr.csr_variant, g_csr.A.view);
            csr_place_output();
            return 0;
        default: return EXIT_FAILURE;  // the ELLPACK operators have no 3-D generator
    }
}

extern "C" int spmv_amd_ellpack_run_device_scaled(const char* mode, const double* d_x, double* d_y,
                                                  double alpha, double beta) {
    switch (which_operator(mode)) {
        case Which::Ell: return ell_run(g_ell, d_x, d_y, alpha, beta);
        case Which::EllStencil: return ell_run(g_ell_stencil, d_x, d_y, alpha, beta);
        default: return EXIT_FAILURE;
    }
}

extern "C" int spmv_amd_download_device_csr(const char* mode, int* row_ptr, int* col_idx,
                                            double* values) {
    CsrBackedOperator* op = which_operator(mode) == Which::Stencil    ? &g_stencil
                            : which_operator(mode) == Which::Csr      ? &g_csr
                            : which_operator(mode) == Which::Stencil7 ? &g_stencil7
                                                                      : nullptr;
    if (!op || !op->ready) return EXIT_FAILURE;
    HIP_CHECK(hipDeviceSynchronize());
    if (row_ptr) download(row_ptr, op->A.row_ptr, (size_t)op->rows + 1);
    if (col_idx) download(col_idx, op->A.col_idx, (size_t)op->A.view.nnz_local);
    if (values) download(values, op->A.values, (size_t)op->A.view.nnz_local);
    return 0;
}

namespace {
// the operator's own staging vectors: what run_timed's kernel reads and writes
bool own_vectors(const char* mode, double** dX, double** dY, size_t* cols, int* candidates, double* gain) {
    switch (which_operator(mode)) {
        case Which::Stencil: *dX = g_stencil.dX, *dY = g_stencil.dY, *cols = (size_t)g_stencil.cols, *candidates = g_stencil.y_candidates, *gain = g_stencil.y_gain; return g_stencil.ready;
        case Which::Csr: *dX = g_csr.dX, *dY = g_csr.dY, *cols = (size_t)g_csr.cols, *candidates = g_csr.y_candidates, *gain = g_csr.y_gain; return g_csr.ready;
        case Which::Stencil7: *dX = g_stencil7.dX, *dY = g_stencil7.dY, *cols = (size_t)g_stencil7.cols, *candidates = g_stencil7.y_candidates, *gain = g_stencil7.y_gain; return g_stencil7.ready;
        case Which::Ell: *dX = g_ell.dX, *dY = g_ell.dY, *cols = (size_t)g_ell.cols, *candidates = g_ell.y_candidates, *gain = g_ell.y_gain; return g_ell.ready;
        case Which::EllStencil: *dX = g_ell_stencil.dX, *dY = g_ell_stencil.dY, *cols = (size_t)g_ell_stencil.cols, *candidates = g_ell_stencil.y_candidates, *gain = g_ell_stencil.y_gain; return g_ell_stencil.ready;
        default: return false;
    }
}
}  // namespace

// `reps` launches of the operator's run_device, each timed with events on the default stream (the kernel-only time run_timed
// reports, without its copies). d_x / d_y == NULL: the operator's OWN staging vectors -- the ones run_timed's kernel works on,
// x set to 1.0 (the reference benchmark's input, main.cu:141-144), y placed by the operator at init (device_runtime.hpp).
extern "C" int spmv_amd_time_run_device(const char* mode, const double* d_x, double* d_y, int reps,
                                        float* ms_each) {
    SpmvOperator* op = get_operator(mode);
    if (!op || reps <= 0) return EXIT_FAILURE;
    if (d_x == nullptr || d_y == nullptr) {
        double *ox = nullptr, *oy = nullptr;
        size_t cols = 0;
        int cand = 0;
        double gain = 0.0;
        if (!own_vectors(mode, &ox, &oy, &cols, &cand, &gain)) return EXIT_FAILURE;
        if (d_x == nullptr) {
            launch_fill(ox, cols, 1.0, kDefaultStream);
            d_x = ox;
        }
        if (d_y == nullptr) d_y = oy;
    }
    EventTimer t;
    for (int i = 0; i < reps; ++i) {
        t.begin(kDefaultStream);
        if (op->run_device(d_x, d_y) != 0) return EXIT_FAILURE;
        t.end(kDefaultStream);
        ms_each[i] = t.elapsed_ms();
    }
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Output placement of an initialised operator: how many allocations were timed for its y vector and what the choice was worth
// (kernel time on the first candidate / on the one kept). 0 = unknown operator or not initialised.
extern "C" int spmv_amd_operator_placement(const char* mode, int* candidates, double* gain) {
    double *ox = nullptr, *oy = nullptr;
    size_t cols = 0;
    int cand = 0;
    double g = 0.0;
    if (!own_vectors(mode, &ox, &oy, &cols, &cand, &g)) return 0;
    if (candidates) *candidates = cand;
    if (gain) *gain = g;
    return 1;
}

extern "C" const char* spmv_amd_operator_variant(const char* mode) {
    switch (which_operator(mode)) {
        case Which::Stencil: return g_stencil.variant_name;
        case Which::Csr: return g_csr.variant_name;
        case Which::Stencil7: return g_stencil7.variant_name;
        case Which::Ell: return g_ell.variant_name;
        case Which::EllStencil: return g_ell_stencil.variant_name;
        default: return "unknown-operator";
    }
}

extern "C" int spmv_amd_operator_select_variant(const char* mode, const char* variant) {
    const bool automatic = variant == nullptr || !strcmp(variant, "auto");
    switch (which_operator(mode)) {
        case Which::Stencil:
            if (automatic) g_stencil.stencil_variant = Stencil5Variant::Auto;
            else if (!strcmp(variant, "row-lds")) g_stencil.stencil_variant = Stencil5Variant::RowLds;
            else if (!strcmp(variant, "row-direct")) g_stencil.stencil_variant = Stencil5Variant::RowDirect;
            else if (!strcmp(variant, "row-generic")) g_stencil.stencil_variant = Stencil5Variant::RowGeneric;
            else return EXIT_FAILURE;
            if (g_stencil.ready) stencil_pick_variant();
            return 0;
        case Which::Stencil7:
            if (automatic) g_stencil7.stencil7_variant = Stencil7Variant::Auto;
            else if (!strcmp(variant, "row-lds")) g_stencil7.stencil7_variant = Stencil7Variant::RowLds;
            else if (!strcmp(variant, "row-direct")) g_stencil7.stencil7_variant = Stencil7Variant::RowDirect;
            else if (!strcmp(variant, "csr-loop")) g_stencil7.stencil7_variant = Stencil7Variant::CsrLoop;
            else return EXIT_FAILURE;
            if (g_stencil7.ready) stencil7_pick_variant();
            return 0;
        case Which::Csr: {
            CsrVariant v;
            if (automatic) v = CsrVariant::Auto;
            else if (!strcmp(variant, "stream")) v = CsrVariant::Stream;
            else if (!strcmp(variant, "adaptive")) v = CsrVariant::Adaptive;
            else if (!strcmp(variant, "row-scalar")) v = CsrVariant::RowScalar;
            else if (!strcmp(variant, "wavefront")) v = CsrVariant::Wavefront;
            else return EXIT_FAILURE;
            g_csr.csr_variant = v;
            if (g_csr.ready) {
                g_csr.variant_name = csr_variant_name(v, g_csr.A.view);
            }
            return 0;
        }
        case Which::Ell:
        case Which::EllStencil: {
            // one kernel each: "auto" only
            if (!automatic) return EXIT_FAILURE;
            EllOperator& e = which_operator(mode) == Which::Ell ? g_ell : g_ell_stencil;
            if (e.ready) e.pick();
            return 0;
        }
        default: return EXIT_FAILURE;
    }
}
