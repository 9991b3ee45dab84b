"""ctypes binding of libspmv_amd.so, used by tests/, bench.py and __graft_entry__.py.

This module is plumbing only: every compute call goes through the C-ABI declared in
include/spmv_amd/api.h into hand-written HIP kernels. There is no CPU fallback; if the
library has not been built, or no GPU is visible when a compute entry point is called, the
call fails loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# The LAB build: the same sources with the test and measurement hooks compiled in (include/spmv_amd/lab.h). A second instance of
# this module bound to it: use_lab() below (tests' `Blab` fixture, tools/, bench.py's scaling probe).
LAB_LIB_PATH = os.path.join(PKG_DIR, "lib", "libspmv_amd_lab.so")
# SPMV_AMD_LIB: measurement aid, lets another build of the library be loaded instead ("lab" = the LAB build)
LIB_PATH = os.environ.get("SPMV_AMD_LIB") or os.path.join(PKG_DIR, "lib", "libspmv_amd.so")
if LIB_PATH == "lab":
    LIB_PATH = LAB_LIB_PATH

ENTRY_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("value", np.float64)], align=True)
assert ENTRY_DTYPE.itemsize == 16
COMM_ID_BYTES = 256


# ---------------------------------------------------------------- structs (include/spmv_amd/types.h)
class MatrixData(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("nnz", C.c_int), ("grid_size", C.c_int), ("entries", C.c_void_p)]


class CSRMatrix(C.Structure):
    _fields_ = [("nb_rows", C.c_int), ("nb_cols", C.c_int), ("nb_nonzeros", C.c_int), ("row_ptr", C.POINTER(C.c_int)), ("col_indices", C.POINTER(C.c_int)), ("values", C.POINTER(C.c_double))]


class ELLPACKMatrix(C.Structure):
    _fields_ = [("nb_rows", C.c_int), ("nb_cols", C.c_int), ("ell_width", C.c_int), ("grid_size", C.c_int), ("indices", C.POINTER(C.c_int)), ("nb_nonzeros", C.c_int), ("values", C.POINTER(C.c_double))]


INIT_FN = C.CFUNCTYPE(C.c_int, C.POINTER(MatrixData))
RUN_TIMED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double))
RUN_DEVICE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
FREE_FN = C.CFUNCTYPE(None)


class SpmvOperator(C.Structure):
    _fields_ = [("name", C.c_char_p), ("init", INIT_FN), ("run_timed", RUN_TIMED_FN), ("run_device", RUN_DEVICE_FN), ("free", FREE_FN)]


class BenchmarkStats(C.Structure):
    _fields_ = [("median_ms", C.c_double), ("mean_ms", C.c_double), ("std_dev_ms", C.c_double), ("min_ms", C.c_double), ("max_ms", C.c_double), ("valid_runs", C.c_int), ("outliers_removed", C.c_int)]


class CGConfig(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("tolerance", C.c_double), ("verbose", C.c_int), ("enable_detailed_timers", C.c_int)]


class CGStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("residual_norm", C.c_double), ("time_total_ms", C.c_double), ("time_spmv_ms", C.c_double), ("time_blas1_ms", C.c_double), ("time_reductions_ms", C.c_double), ("converged", C.c_int), ("solution_sum", C.c_double), ("solution_norm", C.c_double)]


CGConfigMultiGPU = CGConfig  # same layout (include/spmv_amd/types.h)


class CGStatsMultiGPU(C.Structure):
    _fields_ = [
        ("iterations", C.c_int), ("residual_norm", C.c_double), ("time_total_ms", C.c_double), ("time_spmv_ms", C.c_double),
        ("time_blas1_ms", C.c_double), ("time_reductions_ms", C.c_double), ("time_allreduce_ms", C.c_double),
        ("time_allgather_ms", C.c_double), ("converged", C.c_int), ("time_dot_rs_initial_ms", C.c_double),
        ("time_dot_pAp_ms", C.c_double), ("time_dot_rs_new_ms", C.c_double), ("time_axpy_update_x_ms", C.c_double),
        ("time_axpy_update_r_ms", C.c_double), ("time_axpby_update_p_ms", C.c_double), ("time_initial_r_ms", C.c_double),
        ("solution_sum", C.c_double), ("solution_norm", C.c_double),
    ]


class PcgScalars(C.Structure):
    """SpmvAmdPcgScalars (include/spmv_amd/lab.h): the device scalars of one preconditioned solve."""
    _fields_ = [("rz", C.c_double), ("pAp", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("b_norm", C.c_double),
                ("residual", C.c_double), ("iterations", C.c_int), ("converged", C.c_int), ("breakdown", C.c_int), ("skip_update", C.c_int)]


class PcgStageArgs(C.Structure):
    """SpmvAmdPcgStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_pcg_stage call."""
    _fields_ = [("n", C.c_size_t), ("b", C.c_void_p), ("Ap", C.c_void_p), ("dinv", C.c_void_p), ("r", C.c_void_p), ("p", C.c_void_p),
                ("x", C.c_void_p), ("partials", C.c_void_p), ("count", C.c_int), ("which", C.c_int), ("tol", C.c_double),
                ("hist", C.c_void_p), ("hist_cap", C.c_int)]


class MgStageArgs(C.Structure):
    """SpmvAmdMgStageArgs (include/spmv_amd/lab.h): device pointers of one spmv_amd_mg_stage call; n = the fine grid."""
    _fields_ = [("n", C.c_int), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p), ("values", C.c_void_p), ("z", C.c_void_p),
                ("r", C.c_void_p), ("coarse", C.c_void_p), ("out_row_ptr", C.c_void_p), ("out_col_idx", C.c_void_p), ("out_values", C.c_void_p)]


class AmgStageArgs(C.Structure):
    """SpmvAmdAmgStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_amg_stage call."""
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("coarse_rows", C.c_int), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p),
                ("values", C.c_void_p), ("agg_ptr", C.c_void_p), ("members", C.c_void_p), ("agg", C.c_void_p), ("z", C.c_void_p),
                ("r", C.c_void_p), ("coarse", C.c_void_p)]


class MgMultiStageArgs(C.Structure):
    """SpmvAmdMgMultiStageArgs (include/spmv_amd/lab.h): device pointers of one spmv_amd_mg_multi_stage call; n = the fine grid."""
    _fields_ = [("n", C.c_int), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p), ("values", C.c_void_p), ("z", C.c_void_p),
                ("r", C.c_void_p), ("coarse", C.c_void_p), ("d", C.c_void_p), ("dinv", C.c_void_p), ("c0", C.c_double), ("cols", C.c_void_p)]


class MultiColumn(C.Structure):
    """SpmvAmdMultiColumn (include/spmv_amd/lab.h): the per-column state of a batched CG solve."""
    _fields_ = [("rr_old", C.c_double), ("pAp", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("b_norm", C.c_double),
                ("residual", C.c_double), ("active", C.c_int), ("done", C.c_int), ("iterations", C.c_int), ("pad", C.c_int)]


class CgMultiStageArgs(C.Structure):
    """SpmvAmdCgMultiStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_cg_multi_stage call."""
    _fields_ = [("mode", C.c_char_p), ("n", C.c_size_t), ("X", C.c_void_p), ("R", C.c_void_p), ("P", C.c_void_p), ("AP", C.c_void_p),
                ("cols", C.c_void_p), ("partials", C.c_void_p), ("count", C.c_longlong), ("which", C.c_int), ("tol", C.c_double),
                ("hist", C.c_void_p), ("hist_cap", C.c_int), ("xcd_run", C.c_int)]


class PcgMultiColumn(C.Structure):
    """SpmvAmdPcgMultiColumn (include/spmv_amd/lab.h): the per-column state of a batched preconditioned solve."""
    _fields_ = [("rz", C.c_double), ("pAp", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("b_norm", C.c_double),
                ("residual", C.c_double), ("active", C.c_int), ("done", C.c_int), ("iterations", C.c_int), ("converged", C.c_int),
                ("breakdown", C.c_int), ("skip_update", C.c_int), ("pad", C.c_int * 2)]


class PcgMultiStageArgs(C.Structure):
    """SpmvAmdPcgMultiStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_pcg_multi_stage call."""
    _fields_ = [("n", C.c_size_t), ("X", C.c_void_p), ("R", C.c_void_p), ("P", C.c_void_p), ("AP", C.c_void_p), ("D", C.c_void_p),
                ("Z", C.c_void_p), ("dinv", C.c_void_p), ("cols", C.c_void_p), ("partials", C.c_void_p), ("count", C.c_longlong),
                ("which", C.c_int), ("tol", C.c_double), ("hist", C.c_void_p), ("hist_cap", C.c_int), ("c0", C.c_double), ("g", C.c_double),
                ("h", C.c_double), ("last", C.c_int)]


HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int))
BARRIER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)

# Every extern "C" symbol include/spmv_amd/api.h declares (the CPU test-suite checks them all).
DECLARED_SYMBOLS = [
    "csr_mat", "ellpack_matrix", "build_ellpack_from_csr_local", "ensure_ellpack_structure_built", "get_operator",
    "calculate_spmv_metrics", "get_gpu_properties", "print_benchmark_metrics", "print_metrics_json", "print_metrics_csv",
    "read_matrix_type", "read_matrix_general", "read_matrix_symtogen", "load_matrix_market", "convert_csr_to_ellpack",
    "write_matrix_market_stencil5", "write_matrix_market_stencil7", "benchmark_with_stats", "cg_benchmark_with_stats_device",
    "cg_benchmark_with_stats_mgpu_partitioned", "export_cg_json", "export_cg_mgpu_json", "export_cg_csv",
    "spmv_amd_build_csr_struct", "spmv_amd_build_ellpack_from_csr_struct", "spmv_amd_cg_solve", "spmv_amd_cg_solve_device",
    "spmv_amd_cg_solve_mgpu_partitioned", "spmv_amd_reset_host_matrices", "spmv_amd_interior_csr_offset",
    "spmv_amd_partition_rows", "spmv_amd_device_count", "spmv_amd_set_device", "spmv_amd_current_device", "spmv_amd_stream_ceiling", "spmv_amd_stream_ceiling_mix", "spmv_amd_device_alloc", "spmv_amd_device_free",
    "spmv_amd_copy_to_device", "spmv_amd_copy_to_host", "spmv_amd_device_fill_f64", "spmv_amd_device_synchronize",
    "spmv_amd_init_stencil5_synthetic", "spmv_amd_init_stencil7_synthetic", "spmv_amd_init_stencil7_synthetic_values", "spmv_amd_stencil7_row_start", "spmv_amd_ellpack_run_device_scaled", "spmv_amd_download_device_csr", "spmv_amd_time_run_device", "spmv_amd_operator_variant",
    "spmv_amd_operator_select_variant", "spmv_amd_cg_last_history", "spmv_amd_comm_unique_id", "spmv_amd_comm_create_rccl",
    "spmv_amd_comm_create_staged", "spmv_amd_comm_destroy", "spmv_amd_comm_set_world", "spmv_amd_comm_rank", "spmv_amd_comm_size", "spmv_amd_comm_selftest",
    "spmv_amd_comm_barrier", "spmv_amd_comm_transport", "spmv_amd_comm_transport_ranks",
    "spmv_amd_comm_mailbox_enable", "spmv_amd_comm_mailbox_prepare", "spmv_amd_comm_mailbox_connect", "spmv_amd_comm_mailbox_selftest",
    "spmv_amd_comm_mailbox_disable", "spmv_amd_comm_mailbox_ready",
    "spmv_amd_cg_slab_create", "spmv_amd_cg_slab_create_stencil5", "spmv_amd_cg_slab_set_vectors", "spmv_amd_cg_slab_solve",
    "spmv_amd_cg_slab_gather", "spmv_amd_cg_slab_loop_shape", "spmv_amd_cg_slab_history", "spmv_amd_cg_slab_spmv", "spmv_amd_cg_slab_info",
    "spmv_amd_cg_slab_time_spmv", "spmv_amd_cg_slab_set_timeline", "spmv_amd_operator_placement", "spmv_amd_cg_slab_placement", "spmv_amd_cg_slab_tile_runs", "spmv_amd_cg_slab_setup_ms", "spmv_amd_cg_slab_coefficient_form", "spmv_amd_cg_slab_uniform_tiles", "spmv_amd_cg_slab_spmv_launch_ms",  "spmv_amd_cg_release_workspace", "spmv_amd_cg_slab_timeline_names", "spmv_amd_cg_slab_timeline", "spmv_amd_cg_slab_variant", "spmv_amd_cg_slab_destroy", "spmv_amd_version", "spmv_amd_write_stencil5_values",
    "spmv_amd_blas1_axpy", "spmv_amd_blas1_axpby", "spmv_amd_blas1_axpy_dev", "spmv_amd_blas1_update_p_dev", "spmv_amd_blas1_dot",
    "spmv_amd_cg_fused_step",
    "spmv_amd_spmm_device", "spmv_amd_spmm_variant", "spmv_amd_block_to_device", "spmv_amd_block_to_host",
    "spmv_amd_cg_solve_device_multi", "spmv_amd_cg_last_history_multi", "spmv_amd_cg_multi_workspace_bytes",
    "spmv_amd_precond_create", "spmv_amd_precond_create_from_diagonal", "spmv_amd_precond_destroy", "spmv_amd_precond_kind",
    "spmv_amd_precond_inverse_diagonal", "spmv_amd_pcg_solve_device", "spmv_amd_pcg_last_history", "spmv_amd_pcg_release_workspace",
    "spmv_amd_precond_create_chebyshev", "spmv_amd_precond_chebyshev_info", "spmv_amd_precond_apply_device",
    "spmv_amd_precond_create_multigrid", "spmv_amd_precond_multigrid_info",
    "spmv_amd_precond_create_multigrid3d", "spmv_amd_precond_multigrid_dimension",
    "spmv_amd_pcg_solve_device_multi", "spmv_amd_pcg_last_history_multi", "spmv_amd_pcg_multi_workspace_bytes",
    "spmv_amd_precond_create_multigrid_multi", "spmv_amd_precond_multigrid_max_rhs", "spmv_amd_precond_apply_device_multi",
    "spmv_amd_precond_create_multigrid3d_multi",
    "spmv_amd_precond_create_amg", "spmv_amd_precond_amg_info", "spmv_amd_precond_create_amg_multi",
    "spmv_amd_bicgstab_solve_device", "spmv_amd_bicgstab_last_history",
    "spmv_amd_bicgstab_solve_device_multi", "spmv_amd_bicgstab_last_history_multi", "spmv_amd_bicgstab_multi_workspace_bytes",
    "spmv_amd_gcr_solve_device", "spmv_amd_gcr_last_history", "spmv_amd_gcr_workspace_bytes",
    "spmv_amd_gcr_solve_device_multi", "spmv_amd_gcr_last_history_multi", "spmv_amd_gcr_multi_workspace_bytes",
]
# What the LAB build exports on top of that (include/spmv_amd/lab.h); the product library must NOT have these.
LAB_ONLY_SYMBOLS = ["spmv_amd_cg_slab_create_stencil5_as", "spmv_amd_cg_slab_set_option", "spmv_amd_cg_slab_tile_classes", "spmv_amd_cg_slab_block_map", "spmv_amd_cg_slab_slow_blocks",
                    "spmv_amd_cg_slab_direction_spmv", "spmv_amd_cg_slab_spmv_dot", "spmv_amd_cg_slab_initial_stage", "spmv_amd_cg_slab_first_stage", "spmv_amd_cg_slab_stored_b", "spmv_amd_cg_slab_update_r_stage", "spmv_amd_cg_slab_ap_form", "spmv_amd_cg_slab_update_r_from_stage", "spmv_amd_cg_slab_first_recompute_form", "spmv_amd_pcg_stage",
                    "spmv_amd_pcg_last_step_launches", "spmv_amd_cg_multi_stage",
                    "spmv_amd_pcg_last_multigrid_cycles", "spmv_amd_precond_multigrid_level_csr", "spmv_amd_mg_stage",
                    "spmv_amd_amg_stage", "spmv_amd_precond_amg_level_aggregates", "spmv_amd_amg_multi_stage",
                    "spmv_amd_pcg_multi_stage", "spmv_amd_mg_multi_stage", "spmv_amd_mg_multi_stage3d",
                    "spmv_amd_mg3d_multi_level_product", "spmv_amd_precond_multigrid_level_spmm",
                    "spmv_amd_bicgstab_stage", "spmv_amd_gcr_stage", "spmv_amd_operator_fused_spmv", "spmv_amd_bicgstab_multi_stage",
                    "spmv_amd_gcr_multi_stage"]
# C++-linkage entry points kept under the reference's own names (Itanium-mangled).
DECLARED_CXX_SYMBOLS = [
    "SPMV_CSR", "SPMV_STENCIL5_CSR", "SPMV_STENCIL7_CSR", "SPMV_STENCIL_HALO_MGPU", "SPMV_ELLPACK", "SPMV_STENCIL5_ELLPACK",
    "_Z16build_csr_structP10MatrixData",
    "_Z29build_ellpack_from_csr_structPK9CSRMatrixP13ELLPACKMatrixPi",
    "_Z8cg_solveP12SpmvOperatorP10MatrixDataPKdPd8CGConfigP7CGStats",
    "_Z15cg_solve_deviceP12SpmvOperatorP10MatrixDataPKdPd8CGConfigP7CGStats",
    "_Z25cg_solve_mgpu_partitionedP12SpmvOperatorP10MatrixDataPKdPd16CGConfigMultiGPUP15CGStatsMultiGPU",
]


def build(force=False):
    """Compiles libspmv_amd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", PKG_DIR, "clean"], stdout=subprocess.DEVNULL)
    done = subprocess.run(["make", "-C", PKG_DIR, "-j8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if done.returncode != 0:
        raise RuntimeError(f"building libspmv_amd.so failed (make exit {done.returncode}); compiler output:\n{done.stdout[-8000:]}")
    for path in (LIB_PATH, LAB_LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(f"{os.path.basename(path)} was not produced by the build")


_lib = None


def lib():
    """The loaded library. Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    L.get_operator.restype = C.POINTER(SpmvOperator)
    L.get_operator.argtypes = [C.c_char_p]
    L.spmv_amd_version.restype = C.c_char_p
    L.spmv_amd_operator_variant.restype = C.c_char_p
    L.spmv_amd_operator_variant.argtypes = [C.c_char_p]
    L.spmv_amd_operator_select_variant.argtypes = [C.c_char_p, C.c_char_p]
    L.spmv_amd_device_alloc.restype = C.c_void_p
    L.spmv_amd_device_alloc.argtypes = [C.c_size_t]
    L.spmv_amd_device_free.argtypes = [C.c_void_p]
    L.spmv_amd_blas1_axpy.argtypes = [C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]
    L.spmv_amd_blas1_axpby.argtypes = [C.c_size_t, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    L.spmv_amd_blas1_axpy_dev.argtypes = [C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
    L.spmv_amd_blas1_update_p_dev.argtypes = [C.c_size_t, C.c_void_p, C.c_double, C.c_void_p]
    L.spmv_amd_blas1_dot.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.spmv_amd_cg_fused_step.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    L.spmv_amd_current_device.argtypes = [C.c_char_p, C.c_int]
    L.spmv_amd_stream_ceiling.restype = C.c_double
    L.spmv_amd_stream_ceiling.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.spmv_amd_stream_ceiling_mix.restype = C.c_double
    L.spmv_amd_stream_ceiling_mix.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.spmv_amd_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.spmv_amd_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.spmv_amd_device_fill_f64.argtypes = [C.c_void_p, C.c_size_t, C.c_double]
    L.spmv_amd_init_stencil5_synthetic.argtypes = [C.c_char_p, C.c_int]
    L.spmv_amd_init_stencil7_synthetic.argtypes = [C.c_char_p, C.c_int]
    L.spmv_amd_init_stencil7_synthetic_values.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_double]
    L.spmv_amd_stencil7_row_start.argtypes = [C.c_longlong, C.c_int]
    L.spmv_amd_stencil7_row_start.restype = C.c_longlong
    L.write_matrix_market_stencil7.argtypes = [C.c_int, C.c_char_p]
    L.spmv_amd_download_device_csr.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.spmv_amd_ellpack_run_device_scaled.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double]
    L.spmv_amd_time_run_device.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.spmv_amd_cg_solve.argtypes = [C.POINTER(SpmvOperator), C.POINTER(MatrixData), C.c_void_p, C.c_void_p, C.POINTER(CGConfig), C.POINTER(CGStats)]
    L.spmv_amd_cg_solve_device.argtypes = L.spmv_amd_cg_solve.argtypes
    L.spmv_amd_cg_solve_mgpu_partitioned.argtypes = [C.POINTER(MatrixData), C.c_void_p, C.c_void_p, C.POINTER(CGConfig), C.POINTER(CGStatsMultiGPU)]
    L.spmv_amd_cg_last_history.argtypes = [C.c_void_p, C.c_int]
    L.spmv_amd_comm_unique_id.argtypes = [C.c_void_p]
    L.spmv_amd_comm_create_rccl.restype = C.c_void_p
    L.spmv_amd_comm_create_rccl.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.spmv_amd_comm_create_staged.restype = C.c_void_p
    L.spmv_amd_comm_create_staged.argtypes = [C.c_int, C.c_int, HALO_FN, ALLREDUCE_FN, GATHER_FN, BARRIER_FN, C.c_void_p]
    L.spmv_amd_comm_destroy.argtypes = [C.c_void_p]
    L.spmv_amd_comm_set_world.argtypes = [C.c_void_p]
    L.spmv_amd_comm_rank.argtypes = [C.c_void_p]
    L.spmv_amd_comm_size.argtypes = [C.c_void_p]
    L.spmv_amd_comm_selftest.argtypes = [C.c_void_p]
    L.spmv_amd_comm_barrier.argtypes = [C.c_void_p]
    L.spmv_amd_comm_mailbox_enable.argtypes = [C.c_void_p]
    L.spmv_amd_comm_mailbox_prepare.argtypes = [C.c_void_p, C.c_void_p]
    L.spmv_amd_comm_mailbox_connect.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.spmv_amd_comm_mailbox_selftest.argtypes = [C.c_void_p, C.c_int]
    L.spmv_amd_comm_mailbox_disable.argtypes = [C.c_void_p]
    L.spmv_amd_comm_mailbox_ready.argtypes = [C.c_void_p]
    L.spmv_amd_comm_transport.restype = C.c_char_p
    L.spmv_amd_comm_transport.argtypes = [C.c_void_p]
    L.spmv_amd_comm_transport_ranks.argtypes = [C.c_void_p]
    if hasattr(L, "spmv_amd_cg_slab_create_stencil5_as"):  # LAB build only
        L.spmv_amd_cg_slab_create_stencil5_as.restype = C.c_void_p
        L.spmv_amd_cg_slab_create_stencil5_as.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.spmv_amd_cg_slab_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.spmv_amd_cg_slab_set_option.restype = C.c_int
        L.spmv_amd_cg_slab_tile_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
        L.spmv_amd_cg_slab_tile_classes.restype = C.c_longlong
        L.spmv_amd_cg_slab_block_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.spmv_amd_cg_slab_block_map.restype = C.c_longlong
        L.spmv_amd_cg_slab_slow_blocks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.spmv_amd_cg_slab_slow_blocks.restype = C.c_longlong
        L.spmv_amd_cg_slab_direction_spmv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_double), C.c_void_p, C.c_int]
        L.spmv_amd_cg_slab_direction_spmv.restype = C.c_int
        L.spmv_amd_cg_slab_spmv_dot.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int]
        L.spmv_amd_cg_slab_spmv_dot.restype = C.c_int
        L.spmv_amd_cg_slab_initial_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.spmv_amd_cg_slab_initial_stage.restype = C.c_int
        L.spmv_amd_cg_slab_first_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.spmv_amd_cg_slab_first_stage.restype = C.c_int
        L.spmv_amd_cg_slab_stored_b.argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_amd_cg_slab_stored_b.restype = C.c_int
        L.spmv_amd_cg_slab_update_r_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_int]
        L.spmv_amd_cg_slab_update_r_stage.restype = C.c_int
        L.spmv_amd_cg_slab_ap_form.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.spmv_amd_cg_slab_ap_form.restype = C.c_int
        L.spmv_amd_cg_slab_update_r_from_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.spmv_amd_cg_slab_update_r_from_stage.restype = C.c_int
        L.spmv_amd_cg_slab_first_recompute_form.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.spmv_amd_cg_slab_first_recompute_form.restype = C.c_int
        L.spmv_amd_pcg_stage.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PcgStageArgs), C.POINTER(PcgScalars)]
        L.spmv_amd_pcg_stage.restype = C.c_int
        L.spmv_amd_pcg_last_step_launches.argtypes = []
        L.spmv_amd_pcg_last_step_launches.restype = C.c_int
        L.spmv_amd_cg_multi_stage.argtypes = [C.c_char_p, C.c_int, C.POINTER(CgMultiStageArgs)]
        L.spmv_amd_cg_multi_stage.restype = C.c_int
        L.spmv_amd_pcg_last_multigrid_cycles.argtypes = []
        L.spmv_amd_pcg_last_multigrid_cycles.restype = C.c_int
        L.spmv_amd_precond_multigrid_level_csr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_amd_precond_multigrid_level_csr.restype = C.c_int
        L.spmv_amd_mg_stage.argtypes = [C.c_char_p, C.POINTER(MgStageArgs)]
        L.spmv_amd_mg_stage.restype = C.c_int
        L.spmv_amd_amg_stage.argtypes = [C.c_char_p, C.POINTER(AmgStageArgs)]
        L.spmv_amd_amg_stage.restype = C.c_int
        L.spmv_amd_precond_amg_level_aggregates.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.spmv_amd_precond_amg_level_aggregates.restype = C.c_int
        L.spmv_amd_pcg_multi_stage.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(PcgMultiStageArgs)]
        L.spmv_amd_pcg_multi_stage.restype = C.c_int
        L.spmv_amd_mg_multi_stage3d.argtypes = [C.c_char_p, C.c_int, C.POINTER(MgMultiStageArgs)]
        L.spmv_amd_mg_multi_stage3d.restype = C.c_int
        L.spmv_amd_mg3d_multi_level_product.argtypes = [C.c_char_p]
        L.spmv_amd_mg3d_multi_level_product.restype = C.c_int
        L.spmv_amd_precond_multigrid_level_spmm.argtypes = [C.c_void_p, C.c_int]
        L.spmv_amd_precond_multigrid_level_spmm.restype = C.c_char_p
        L.spmv_amd_operator_fused_spmv.argtypes = [C.POINTER(SpmvOperator), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_operator_fused_spmv.restype = C.c_int
    L.spmv_amd_cg_slab_create.restype = C.c_void_p
    L.spmv_amd_cg_slab_create.argtypes = [C.POINTER(MatrixData), C.c_void_p]
    L.spmv_amd_cg_slab_create_stencil5.restype = C.c_void_p
    L.spmv_amd_cg_slab_create_stencil5.argtypes = [C.c_int, C.c_void_p]
    L.spmv_amd_cg_slab_set_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.spmv_amd_cg_slab_solve.argtypes = [C.c_void_p, C.POINTER(CGConfig), C.POINTER(CGStatsMultiGPU)]
    L.spmv_amd_cg_slab_gather.argtypes = [C.c_void_p, C.c_void_p]
    L.spmv_amd_cg_slab_history.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.spmv_amd_cg_slab_spmv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.spmv_amd_cg_slab_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.spmv_amd_cg_slab_time_spmv.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.spmv_amd_cg_slab_destroy.argtypes = [C.c_void_p]
    L.spmv_amd_cg_slab_set_timeline.argtypes = [C.c_void_p, C.c_int]
    L.spmv_amd_cg_slab_set_timeline.restype = None
    L.spmv_amd_cg_slab_timeline_names.restype = C.c_char_p
    L.spmv_amd_cg_slab_timeline.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.spmv_amd_cg_slab_variant.restype = C.c_char_p
    L.spmv_amd_cg_slab_variant.argtypes = [C.c_void_p]
    L.spmv_amd_cg_slab_coefficient_form.argtypes = [C.c_void_p]
    L.spmv_amd_cg_slab_coefficient_form.restype = C.c_int
    L.spmv_amd_cg_slab_uniform_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.spmv_amd_cg_slab_uniform_tiles.restype = C.c_int
    L.spmv_amd_cg_slab_loop_shape.restype = C.c_char_p
    L.spmv_amd_cg_slab_loop_shape.argtypes = [C.c_void_p]
    L.load_matrix_market.argtypes = [C.c_char_p, C.POINTER(MatrixData)]
    L.write_matrix_market_stencil5.argtypes = [C.c_int, C.c_char_p]
    L.spmv_amd_write_stencil5_values.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p]
    L.read_matrix_type.argtypes = [C.c_char_p]
    L.spmv_amd_partition_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.benchmark_with_stats.argtypes = [RUN_TIMED_FN, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(BenchmarkStats)]
    _lib = L
    return L


def is_lab():
    """True when the loaded library is the LAB build (it has the hooks of include/spmv_amd/lab.h)."""
    return hasattr(lib(), "spmv_amd_cg_slab_set_option")


def use_lab():
    """A SECOND instance of this module bound to the LAB build (this one stays on the product library). Both libraries can be
    loaded in one process: each has its own globals (ctypes loads them RTLD_LOCAL)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("spmv_amd_binding_lab", os.path.abspath(__file__))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LIB_PATH = LAB_LIB_PATH
    return mod


def require_gpu():
    if lib().spmv_amd_device_count() < 1:
        raise RuntimeError("no HIP device visible: libspmv_amd has no CPU path")


def current_device():
    """(device index, PCI bus id) of the calling thread's current HIP device."""
    buf = C.create_string_buffer(64)
    dev = lib().spmv_amd_current_device(buf, 64)
    return dev, buf.value.decode()


def stream_ceiling(rows, warmup=3, reps=20, mix="stencil5"):
    """Per-launch milliseconds and bytes of the stream probe (csrc/stream_ceiling.hip) for a format's byte mix:
    "stencil5" 48:8 B/row, "csr" 72:8 (values, column indices, row pointers, x : y), "ellpack" 68:8, "read-only" 48:0."""
    require_gpu()
    ms = (C.c_float * reps)()
    nbytes = lib().spmv_amd_stream_ceiling_mix({"stencil5": 0, "csr": 1, "ellpack": 2, "read-only": 3}[mix], int(rows), int(warmup), int(reps), ms)
    if nbytes <= 0:
        raise RuntimeError("spmv_amd_stream_ceiling failed")
    return np.array(ms[:], dtype=np.float64), nbytes


def csr_mat():
    return CSRMatrix.in_dll(lib(), "csr_mat")


def ellpack_matrix():
    return ELLPACKMatrix.in_dll(lib(), "ellpack_matrix")


# ---------------------------------------------------------------- host-side helpers
class HostMatrix:
    """A MatrixData whose entries live in a numpy array owned by this object."""

    def __init__(self, entries, rows, cols, grid_size=-1):
        self.entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
        self.c = MatrixData(int(rows), int(cols), len(self.entries), int(grid_size), self.entries.ctypes.data)

    @property
    def ptr(self):
        return C.byref(self.c)


def load_matrix_market(path):
    m = MatrixData()
    rc = lib().load_matrix_market(os.fsencode(path), C.byref(m))
    if rc != 0:
        raise IOError(f"load_matrix_market({path}) -> {rc}")
    e = np.ctypeslib.as_array((C.c_byte * (16 * m.nnz)).from_address(m.entries)).view(ENTRY_DTYPE).copy()
    C.CDLL(None).free(C.c_void_p(m.entries))
    return HostMatrix(e, m.rows, m.cols, m.grid_size)


def read_matrix_symtogen(path):
    """read_matrix_symtogen with every output requested: (rows, cols, stored nnz, expanded nnz, row_ptr, col_idx,
    values, expanded entries). The CSR arrays are the reference reader's (columns in a row in file order)."""
    m = MatrixData()
    rows, cols, nnz, full = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rp, ci, va = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
    lib().read_matrix_symtogen(C.byref(m), os.fsencode(path), C.byref(rows), C.byref(cols), C.byref(nnz), C.byref(rp), C.byref(ci),
                               C.byref(va), C.byref(full))
    if not m.entries:
        raise IOError(f"read_matrix_symtogen({path}) failed")
    out = (rows.value, cols.value, nnz.value, full.value, np.ctypeslib.as_array(rp, shape=(rows.value + 1,)).copy(),
           np.ctypeslib.as_array(ci, shape=(full.value,)).copy(), np.ctypeslib.as_array(va, shape=(full.value,)).copy(),
           np.ctypeslib.as_array((C.c_byte * (16 * m.nnz)).from_address(m.entries)).view(ENTRY_DTYPE).copy())
    libc = C.CDLL(None)
    for ptr in (rp, ci, va, C.c_void_p(m.entries)):
        libc.free(ptr)
    return out


def host_csr_arrays():
    """Copies of the process-wide csr_mat built by build_csr_struct."""
    m = csr_mat()
    rp = np.ctypeslib.as_array(m.row_ptr, shape=(m.nb_rows + 1,)).copy()
    ci = np.ctypeslib.as_array(m.col_indices, shape=(m.nb_nonzeros,)).copy()
    va = np.ctypeslib.as_array(m.values, shape=(m.nb_nonzeros,)).copy()
    return rp, ci, va


def host_ell_arrays():
    m = ellpack_matrix()
    n = m.nb_rows * m.ell_width
    return m.ell_width, np.ctypeslib.as_array(m.indices, shape=(n,)).copy(), np.ctypeslib.as_array(m.values, shape=(n,)).copy()


def partition_rows(n, world, rank):
    off, nl = C.c_int(), C.c_int()
    lib().spmv_amd_partition_rows(n, world, rank, C.byref(off), C.byref(nl))
    return off.value, nl.value


# ---------------------------------------------------------------- device-side helpers
class DeviceVector:
    def __init__(self, count, fill=None):
        self.count = int(count)
        self.ptr = lib().spmv_amd_device_alloc(self.count * 8)
        if fill is not None:
            lib().spmv_amd_device_fill_f64(self.ptr, self.count, float(fill))

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        v = cls(len(a))
        lib().spmv_amd_copy_to_device(v.ptr, a.ctypes.data, a.nbytes)
        return v

    def to_host(self):
        out = np.empty(self.count, dtype=np.float64)
        lib().spmv_amd_device_synchronize()
        lib().spmv_amd_copy_to_host(out.ctypes.data, self.ptr, out.nbytes)
        return out

    def free(self):
        if self.ptr:
            lib().spmv_amd_device_free(self.ptr)
            self.ptr = None


class Operator:
    """get_operator(name) with numpy-friendly wrappers around the vtable."""

    def __init__(self, name):
        self.name = name
        p = lib().get_operator(name.encode())
        if not p:
            raise KeyError(name)
        self.op = p
        self.rows = self.cols = 0

    @property
    def canonical_name(self):
        return self.op.contents.name.decode()

    def init(self, host_matrix):
        require_gpu()
        rc = self.op.contents.init(host_matrix.ptr)
        self.rows, self.cols = host_matrix.c.rows, host_matrix.c.cols
        return rc

    def init_synthetic(self, n):
        require_gpu()
        rc = lib().spmv_amd_init_stencil5_synthetic(self.name.encode(), int(n))
        self.rows = self.cols = n * n
        return rc

    def init_synthetic3d(self, n, center=7.0, off=-1.0):
        """spmv_amd_init_stencil7_synthetic_values: the n x n x n 7-point matrix (centre 7, neighbours -1 by default: the generator
        matrix; 6 / -1 is Poisson) built in HBM ("stencil7-csr", "cusparse-csr")."""
        require_gpu()
        rc = lib().spmv_amd_init_stencil7_synthetic_values(self.name.encode(), int(n), float(center), float(off))
        self.rows = self.cols = n * n * n
        return rc

    def run_timed(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert len(x) == self.cols
        y = np.zeros(self.rows, dtype=np.float64)
        ms = C.c_double()
        rc = self.op.contents.run_timed(x.ctypes.data, y.ctypes.data, C.byref(ms))
        if rc != 0:
            raise RuntimeError(f"run_timed -> {rc}")
        return y, ms.value

    def run_device(self, d_x, d_y):
        return self.op.contents.run_device(d_x.ptr, d_y.ptr)

    def time_device(self, d_x, d_y, reps):
        """Kernel-only ms of `reps` run_device launches; d_x / d_y None = the operator's own staging vectors (x = 1), the
        ones run_timed's kernel works on."""
        ms = (C.c_float * reps)()
        rc = lib().spmv_amd_time_run_device(self.name.encode(), None if d_x is None else d_x.ptr, None if d_y is None else d_y.ptr, reps, ms)
        if rc != 0:
            raise RuntimeError(f"time_run_device -> {rc}")
        return np.array(ms[:], dtype=np.float64)

    def placement(self):
        """(candidates timed for the operator's y vector at init, kernel time on the first / on the one kept)"""
        cand, gain = C.c_int(), C.c_double()
        lib().spmv_amd_operator_placement.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        ok = lib().spmv_amd_operator_placement(self.name.encode(), C.byref(cand), C.byref(gain))
        return (cand.value, gain.value) if ok else None

    def variant(self):
        return lib().spmv_amd_operator_variant(self.name.encode()).decode()

    def select_variant(self, variant):
        return lib().spmv_amd_operator_select_variant(self.name.encode(), None if variant is None else variant.encode())

    def download_csr(self, rows, nnz):
        rp = np.empty(rows + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        va = np.empty(nnz, dtype=np.float64)
        rc = lib().spmv_amd_download_device_csr(self.name.encode(), rp.ctypes.data, ci.ctypes.data, va.ctypes.data)
        assert rc == 0
        return rp, ci, va

    def free(self):
        self.op.contents.free()

    def run_spmm(self, Xk):
        """Y = A X for the k = 1..8 columns of Xk (numpy (k, cols)) through spmv_amd_spmm_device; returns Y (k, rows)."""
        Xk = np.ascontiguousarray(np.atleast_2d(Xk), dtype=np.float64)
        k = Xk.shape[0]
        assert Xk.shape[1] == self.cols
        dx, dy = DeviceBlock.from_host(Xk), DeviceBlock(k, self.rows)
        try:
            rc = _multi_lib().spmv_amd_spmm_device(self.name.encode(), k, dx.ptr, dy.ptr)
            if rc != 0:
                raise RuntimeError(f"spmm_device -> {rc}")
            return dy.to_host()
        finally:
            dx.free(), dy.free()

    def spmm_variant(self):
        return _multi_lib().spmv_amd_spmm_variant(self.name.encode()).decode()


def cg_solve(op, host_matrix, b, x0, max_iters=1000, tol=1e-6, device=True, verbose=0, timers=0):
    """cg_solve_device (device=True) or cg_solve through the C-ABI; returns x, history, stats."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    cfg = CGConfig(max_iters, tol, verbose, timers)
    st = CGStats()
    fn = lib().spmv_amd_cg_solve_device if device else lib().spmv_amd_cg_solve
    rc = fn(op.op, host_matrix.ptr, b.ctypes.data, x.ctypes.data, C.byref(cfg), C.byref(st))
    if rc != 0:
        raise RuntimeError(f"cg_solve -> {rc}")
    hist = np.zeros(max_iters + 1, dtype=np.float64)
    count = lib().spmv_amd_cg_last_history(hist.ctypes.data, len(hist))
    return x, hist[:count].copy(), st


# ---------------------------------------------------------------- several right-hand sides (include/spmv_amd/api.h)
def _multi_lib():
    """lib() with the signatures of the multi-RHS entry points set."""
    L = lib()
    if not getattr(L, "_multi_sigs", False):
        L.spmv_amd_spmm_device.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_amd_spmm_variant.argtypes = [C.c_char_p]
        L.spmv_amd_spmm_variant.restype = C.c_char_p
        L.spmv_amd_block_to_device.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        L.spmv_amd_block_to_host.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        L.spmv_amd_cg_solve_device_multi.argtypes = [C.POINTER(SpmvOperator), C.POINTER(MatrixData), C.c_int, C.c_void_p, C.c_void_p,
                                                     C.POINTER(CGConfig), C.POINTER(CGStats)]
        L.spmv_amd_cg_last_history_multi.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.spmv_amd_cg_multi_workspace_bytes.argtypes = []
        L.spmv_amd_cg_multi_workspace_bytes.restype = C.c_size_t
        L._multi_sigs = True
    return L


class DeviceBlock:
    """k vectors of n rows on the device, row-interleaved (element (row, j) at [row * k + j], api.h); host side (k, n)."""

    def __init__(self, k, n):
        self.k, self.n = int(k), int(n)
        self.ptr = lib().spmv_amd_device_alloc(self.k * self.n * 8)

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
        v = cls(a.shape[0], a.shape[1])
        if _multi_lib().spmv_amd_block_to_device(v.k, v.n, a.ctypes.data, v.ptr) != 0:
            raise RuntimeError("block_to_device failed")
        return v

    def to_host(self):
        out = np.empty((self.k, self.n), dtype=np.float64)
        lib().spmv_amd_device_synchronize()
        if _multi_lib().spmv_amd_block_to_host(self.k, self.n, self.ptr, out.ctypes.data) != 0:
            raise RuntimeError("block_to_host failed")
        return out

    def free(self):
        if self.ptr:
            lib().spmv_amd_device_free(self.ptr)
            self.ptr = None


def cg_solve_multi(op, host_matrix, Bk, X0k, max_iters=1000, tol=1e-6, verbose=0, timers=0):
    """spmv_amd_cg_solve_device_multi: k independent CG solves sharing the SpMM. Bk, X0k: (k, n).
    Returns X (k, n), a list of k residual histories and a list of k CGStats."""
    Bk = np.ascontiguousarray(np.atleast_2d(Bk), dtype=np.float64)
    X = np.ascontiguousarray(np.atleast_2d(X0k), dtype=np.float64).copy()
    k = Bk.shape[0]
    assert X.shape == Bk.shape
    cfg = CGConfig(max_iters, tol, verbose, timers)
    stats = (CGStats * k)()
    L = _multi_lib()
    rc = L.spmv_amd_cg_solve_device_multi(op.op, host_matrix.ptr, k, Bk.ctypes.data, X.ctypes.data, C.byref(cfg), stats)
    if rc != 0:
        raise RuntimeError(f"cg_solve_device_multi -> {rc}")
    hists = []
    for j in range(k):
        h = np.zeros(max_iters + 1, dtype=np.float64)
        count = L.spmv_amd_cg_last_history_multi(j, h.ctypes.data, len(h))
        hists.append(h[:count].copy())
    return X, hists, list(stats)


def cg_multi_stage(stage, k, args):
    """spmv_amd_cg_multi_stage (LAB build only; include/spmv_amd/lab.h): one stage of the batched solver's own kernels on the
    device data `args` (CgMultiStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched-CG stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_cg_multi_stage(stage if stage is None else stage.encode(), int(k), None if args is None else C.byref(args))


# ---------------------------------------------------------------- preconditioned CG (include/spmv_amd/api.h)
def _pcg_lib():
    """lib() with the signatures of the preconditioned-CG entry points set."""
    L = lib()
    if not getattr(L, "_pcg_sigs", False):
        L.spmv_amd_precond_create.argtypes = [C.POINTER(SpmvOperator), C.c_char_p, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create.restype = C.c_void_p
        L.spmv_amd_precond_create_from_diagonal.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_from_diagonal.restype = C.c_void_p
        L.spmv_amd_precond_destroy.argtypes = [C.c_void_p]
        L.spmv_amd_precond_destroy.restype = None
        L.spmv_amd_precond_kind.argtypes = [C.c_void_p]
        L.spmv_amd_precond_kind.restype = C.c_char_p
        L.spmv_amd_precond_inverse_diagonal.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.spmv_amd_pcg_solve_device.argtypes = [C.POINTER(SpmvOperator), C.POINTER(MatrixData), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(CGConfig), C.POINTER(CGStats)]
        L.spmv_amd_pcg_last_history.argtypes = [C.c_void_p, C.c_int]
        L.spmv_amd_pcg_release_workspace.argtypes = []
        L.spmv_amd_pcg_release_workspace.restype = None
        L.spmv_amd_precond_create_chebyshev.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_chebyshev.restype = C.c_void_p
        L.spmv_amd_precond_chebyshev_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                      C.c_void_p, C.c_int]
        L.spmv_amd_precond_apply_device.argtypes = [C.POINTER(SpmvOperator), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.spmv_amd_precond_create_multigrid.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_multigrid.restype = C.c_void_p
        L.spmv_amd_precond_multigrid_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
        L.spmv_amd_precond_create_multigrid3d.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_multigrid3d.restype = C.c_void_p
        L.spmv_amd_precond_multigrid_dimension.argtypes = [C.c_void_p]
        L.spmv_amd_precond_multigrid_dimension.restype = C.c_int
        L.spmv_amd_pcg_solve_device_multi.argtypes = [C.POINTER(SpmvOperator), C.POINTER(MatrixData), C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.POINTER(CGConfig), C.POINTER(CGStats)]
        L.spmv_amd_pcg_last_history_multi.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.spmv_amd_pcg_multi_workspace_bytes.argtypes = []
        L.spmv_amd_pcg_multi_workspace_bytes.restype = C.c_size_t
        L.spmv_amd_precond_create_multigrid_multi.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_multigrid_multi.restype = C.c_void_p
        L.spmv_amd_precond_create_multigrid3d_multi.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_multigrid3d_multi.restype = C.c_void_p
        L.spmv_amd_precond_multigrid_max_rhs.argtypes = [C.c_void_p]
        L.spmv_amd_precond_multigrid_max_rhs.restype = C.c_int
        L.spmv_amd_precond_apply_device_multi.argtypes = [C.POINTER(SpmvOperator), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_amd_precond_create_amg.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_amg.restype = C.c_void_p
        L.spmv_amd_precond_amg_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int]
        L.spmv_amd_precond_create_amg_multi.argtypes = [C.POINTER(SpmvOperator), C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int)]
        L.spmv_amd_precond_create_amg_multi.restype = C.c_void_p
        L._pcg_sigs = True
    return L


class Precond:
    """Owner of an SpmvAmdPrecond handle. Precond(op, kind) or Precond.from_diagonal(d); a refusal raises ValueError with
    .bad_row (the first offending row, or -1)."""

    def __init__(self, op=None, kind="jacobi", _handle=None, _n=0):
        if _handle is None:
            bad = C.c_int(-2)
            _handle = _pcg_lib().spmv_amd_precond_create(op.op, kind.encode(), C.byref(bad))
            if not _handle:
                err = ValueError(f"precond_create({op.name}, {kind}) refused, bad_row = {bad.value}")
                err.bad_row = bad.value
                raise err
            _n = op.rows
        self.handle = _handle
        self.n = _n

    @classmethod
    def from_diagonal(cls, d):
        d = np.ascontiguousarray(d, dtype=np.float64)
        dv = DeviceVector.from_host(d)
        try:
            bad = C.c_int(-2)
            h = _pcg_lib().spmv_amd_precond_create_from_diagonal(dv.ptr, len(d), C.byref(bad))
        finally:
            dv.free()
        if not h:
            err = ValueError(f"precond_create_from_diagonal refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=len(d))

    @classmethod
    def chebyshev(cls, op, degree=4, lambda_min=0.0, lambda_max=0.0):
        """spmv_amd_precond_create_chebyshev; bounds <= 0 ask for the automatic ones."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_chebyshev(op.op, degree, lambda_min, lambda_max, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_chebyshev({op.name}, {degree}, {lambda_min}, {lambda_max}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def multigrid(cls, op, smoother_degree=1, max_levels=0):
        """spmv_amd_precond_create_multigrid (stencil5-csr only); max_levels 0 = automatic."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_multigrid(op.op, smoother_degree, max_levels, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_multigrid({op.name}, {smoother_degree}, {max_levels}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def multigrid3d(cls, op, smoother_degree=1, max_levels=0):
        """spmv_amd_precond_create_multigrid3d (stencil7-csr on a verified 7-point stencil only); max_levels 0 = automatic."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_multigrid3d(op.op, smoother_degree, max_levels, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_multigrid3d({op.name}, {smoother_degree}, {max_levels}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def multigrid_multi(cls, op, smoother_degree=1, max_levels=0, max_rhs=8):
        """spmv_amd_precond_create_multigrid_multi (stencil5-csr only): the hierarchy with block vectors of max_rhs columns."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_multigrid_multi(op.op, smoother_degree, max_levels, max_rhs, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_multigrid_multi({op.name}, {smoother_degree}, {max_levels}, {max_rhs}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def multigrid3d_multi(cls, op, smoother_degree=1, max_levels=0, max_rhs=8):
        """spmv_amd_precond_create_multigrid3d_multi (stencil7-csr on a verified 7-point stencil only): the 3-D hierarchy with block
        vectors of max_rhs columns."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_multigrid3d_multi(op.op, smoother_degree, max_levels, max_rhs, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_multigrid3d_multi({op.name}, {smoother_degree}, {max_levels}, {max_rhs}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def amg(cls, op, smoother_degree=1, max_levels=0, strength=0.08):
        """spmv_amd_precond_create_amg (cusparse-csr only): aggregation AMG from the matrix; max_levels 0 = automatic."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_amg(op.op, smoother_degree, max_levels, strength, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_amg({op.name}, {smoother_degree}, {max_levels}, {strength}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    @classmethod
    def amg_multi(cls, op, smoother_degree=1, max_levels=0, strength=0.08, max_rhs=8):
        """spmv_amd_precond_create_amg_multi (cusparse-csr only): the AMG hierarchy with block vectors of max_rhs columns."""
        bad = C.c_int(-2)
        h = _pcg_lib().spmv_amd_precond_create_amg_multi(op.op, smoother_degree, max_levels, strength, max_rhs, C.byref(bad))
        if not h:
            err = ValueError(f"precond_create_amg_multi({op.name}, {smoother_degree}, {max_levels}, {strength}, {max_rhs}) refused, bad_row = {bad.value}")
            err.bad_row = bad.value
            raise err
        return cls(_handle=h, _n=op.rows)

    def amg_info(self):
        """A dict of an AMG handle -- smoother_degree, strength, setup_ms and per level rows, nnz, max_aggregate, lambda_max --; None
        for any other handle."""
        levels, degree, theta, ms = C.c_int(0), C.c_int(-1), C.c_double(0.0), C.c_double(0.0)
        rows, agg = np.zeros(32, dtype=np.int32), np.zeros(32, dtype=np.int32)
        nnz, lmax = np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.float64)
        count = _pcg_lib().spmv_amd_precond_amg_info(self.handle, C.byref(levels), C.byref(degree), C.byref(theta), rows.ctypes.data,
                                                     nnz.ctypes.data, agg.ctypes.data, lmax.ctypes.data, C.byref(ms), 32)
        if count == 0:
            return None
        return {"smoother_degree": degree.value, "strength": theta.value, "setup_ms": ms.value, "rows": [int(v) for v in rows[:count]],
                "nnz": [int(v) for v in nnz[:count]], "max_aggregate": [int(v) for v in agg[:count]], "lambda_max": lmax[:count].copy()}

    def amg_level(self, level):
        """row_ptr, col_idx, values, dinv and the aggregate map (None on the coarsest level) of one level of an AMG handle (LAB build
        only; include/spmv_amd/lab.h)."""
        if not is_lab():
            raise RuntimeError("the level matrices are read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        info = self.amg_info()
        rows, nnz = info["rows"][level], info["nnz"][level]
        rp, ci = np.zeros(rows + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
        va, dinv = np.zeros(nnz), np.zeros(rows)
        if lib().spmv_amd_precond_multigrid_level_csr(self.handle, level, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, dinv.ctypes.data) != 0:
            raise RuntimeError("precond_multigrid_level_csr refused")
        agg = None
        if level + 1 < len(info["rows"]):
            agg = np.zeros(rows, dtype=np.int32)
            if lib().spmv_amd_precond_amg_level_aggregates(self.handle, level, agg.ctypes.data) != 0:
                raise RuntimeError("precond_amg_level_aggregates refused")
        return rp, ci, va, dinv, agg

    def multigrid_level_spmm(self, level):
        """The name of one level's SpMM plan in a hierarchy with block vectors (LAB build only; include/spmv_amd/lab.h)."""
        if not is_lab():
            raise RuntimeError("the level plans are read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        return lib().spmv_amd_precond_multigrid_level_spmm(self.handle, level).decode()

    def multigrid_max_rhs(self):
        """The columns a multigrid hierarchy's block vectors hold; 0 for a single-vector hierarchy or another kind."""
        return _pcg_lib().spmv_amd_precond_multigrid_max_rhs(self.handle)

    def multigrid_dimension(self):
        """2 or 3 for a multigrid preconditioner, 0 for another kind."""
        return _pcg_lib().spmv_amd_precond_multigrid_dimension(self.handle)

    @property
    def kind(self):
        return _pcg_lib().spmv_amd_precond_kind(self.handle).decode()

    def multigrid_info(self):
        """smoother degree, the levels' grids and their lambda_max; None for another kind."""
        levels, degree = C.c_int(0), C.c_int(-1)
        grids, lmax = np.zeros(32, dtype=np.int32), np.zeros(32, dtype=np.float64)
        count = _pcg_lib().spmv_amd_precond_multigrid_info(self.handle, C.byref(levels), C.byref(degree), grids.ctypes.data, lmax.ctypes.data, 32)
        if count == 0:
            return None
        return degree.value, [int(g) for g in grids[:count]], lmax[:count].copy()

    def multigrid_level(self, level):
        """row_ptr, col_idx, values and dinv of one level (LAB build only; include/spmv_amd/lab.h)."""
        if not is_lab():
            raise RuntimeError("the level matrices are read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        n = self.multigrid_info()[1][level]
        rows, nnz = (n ** 3, 7 * n ** 3 - 6 * n * n) if self.multigrid_dimension() == 3 else (n * n, 5 * n * n - 4 * n)
        rp, ci = np.zeros(rows + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
        va, dinv = np.zeros(nnz), np.zeros(rows)
        if lib().spmv_amd_precond_multigrid_level_csr(self.handle, level, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, dinv.ctypes.data) != 0:
            raise RuntimeError("precond_multigrid_level_csr refused")
        return rp, ci, va, dinv

    def chebyshev_info(self):
        """degree, lambda_min, lambda_max and the coefficients [c0, h_1, g_1, ...]; None for another kind."""
        deg, lo, hi = C.c_int(-1), C.c_double(0.0), C.c_double(0.0)
        coef = np.zeros(65, dtype=np.float64)
        count = _pcg_lib().spmv_amd_precond_chebyshev_info(self.handle, C.byref(deg), C.byref(lo), C.byref(hi), coef.ctypes.data, len(coef))
        if count == 0:
            return None
        return deg.value, lo.value, hi.value, coef[:count].copy()

    def apply_device(self, op, r_ptr, z_ptr):
        """spmv_amd_precond_apply_device on device pointers; returns r.z (raises RuntimeError on a refusal)."""
        rz = C.c_double(0.0)
        if _pcg_lib().spmv_amd_precond_apply_device(op.op, self.handle, r_ptr, z_ptr, C.byref(rz)) != 0:
            raise RuntimeError("precond_apply_device refused")
        return rz.value

    def apply_device_multi(self, op, k, R_ptr, Z_ptr):
        """spmv_amd_precond_apply_device_multi on device pointers of k interleaved columns (raises RuntimeError on a refusal)."""
        if _pcg_lib().spmv_amd_precond_apply_device_multi(op.op, self.handle, int(k), R_ptr, Z_ptr) != 0:
            raise RuntimeError("precond_apply_device_multi refused")

    def inverse_diagonal(self):
        out = np.empty(self.n, dtype=np.float64)
        if _pcg_lib().spmv_amd_precond_inverse_diagonal(self.handle, out.ctypes.data, self.n) != 0:
            raise RuntimeError("precond_inverse_diagonal refused")
        return out

    def destroy(self):
        if self.handle:
            _pcg_lib().spmv_amd_precond_destroy(self.handle)
            self.handle = None


def pcg_solve_device(op, host_matrix, precond, b, x0, max_iters=1000, tol=1e-6, verbose=0, timers=0):
    """spmv_amd_pcg_solve_device; returns x, history, stats (raises RuntimeError on a refusal)."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    cfg = CGConfig(max_iters, tol, verbose, timers)
    st = CGStats()
    L = _pcg_lib()
    rc = L.spmv_amd_pcg_solve_device(op.op, host_matrix.ptr, precond.handle, b.ctypes.data, x.ctypes.data, C.byref(cfg), C.byref(st))
    if rc != 0:
        raise RuntimeError(f"pcg_solve_device -> {rc}")
    hist = np.zeros(max_iters + 1, dtype=np.float64)
    count = L.spmv_amd_pcg_last_history(hist.ctypes.data, len(hist))
    return x, hist[:count].copy(), st


def pcg_solve_multi(op, host_matrix, precond, Bk, X0k, max_iters=1000, tol=1e-6, verbose=0, timers=0):
    """spmv_amd_pcg_solve_device_multi: k independent preconditioned solves sharing the SpMM. Bk, X0k: (k, n).
    Returns X (k, n), a list of k residual histories and a list of k CGStats (raises RuntimeError on a refusal)."""
    Bk = np.ascontiguousarray(np.atleast_2d(Bk), dtype=np.float64)
    X = np.ascontiguousarray(np.atleast_2d(X0k), dtype=np.float64).copy()
    k = Bk.shape[0]
    assert X.shape == Bk.shape
    cfg = CGConfig(max_iters, tol, verbose, timers)
    stats = (CGStats * k)()
    L = _pcg_lib()
    rc = L.spmv_amd_pcg_solve_device_multi(op.op, host_matrix.ptr, precond.handle, k, Bk.ctypes.data, X.ctypes.data, C.byref(cfg), stats)
    if rc != 0:
        raise RuntimeError(f"pcg_solve_device_multi -> {rc}")
    hists = []
    for j in range(k):
        h = np.zeros(max_iters + 1, dtype=np.float64)
        count = L.spmv_amd_pcg_last_history_multi(j, h.ctypes.data, len(h))
        hists.append(h[:count].copy())
    return X, hists, list(stats)


def pcg_multi_stage(stage, kind, k, args):
    """spmv_amd_pcg_multi_stage (LAB build only; include/spmv_amd/lab.h): one stage of the batched preconditioned solver's own
    kernels on the device data `args` (PcgMultiStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched-PCG stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_pcg_multi_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(), int(k),
                                          None if args is None else C.byref(args))


def mg_stage(stage, args):
    """spmv_amd_mg_stage (LAB build only; include/spmv_amd/lab.h): one launch of the multigrid cycle on the caller's device data."""
    if not is_lab():
        raise RuntimeError("the multigrid stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_mg_stage(stage if stage is None else stage.encode(), args)


def amg_stage(stage, args):
    """spmv_amd_amg_stage (LAB build only; include/spmv_amd/lab.h): one of the two launches an AMG level adds to the cycle, on the
    caller's device data `args` (AmgStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the AMG stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_amg_stage(stage if stage is None else stage.encode(), None if args is None else C.byref(args))


def amg_multi_stage(stage, k, args):
    """spmv_amd_amg_multi_stage (LAB build only; include/spmv_amd/lab.h): one of the two launches an AMG level adds to the batched cycle,
    on the caller's device blocks of k columns `args` (AmgStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the AMG stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_amg_multi_stage(stage if stage is None else stage.encode(), int(k), None if args is None else C.byref(args))


def mg_multi_stage(stage, k, args):
    """spmv_amd_mg_multi_stage (LAB build only; include/spmv_amd/lab.h): one launch of the batched multigrid cycle on the caller's
    device data `args` (MgMultiStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched multigrid stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_mg_multi_stage(stage if stage is None else stage.encode(), int(k), None if args is None else C.byref(args))


def mg_multi_stage3d(stage, k, args):
    """spmv_amd_mg_multi_stage3d (LAB build only; include/spmv_amd/lab.h): one of the two launches a 3-D level adds to the batched
    multigrid cycle, on the caller's device data `args` (MgMultiStageArgs, n = the fine grid of n^3 rows) points to; returns its return
    code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched multigrid stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_mg_multi_stage3d(stage if stage is None else stage.encode(), int(k), None if args is None else C.byref(args))


def mg3d_multi_level_product(kind):
    """spmv_amd_mg3d_multi_level_product (LAB build only): "auto", "csr" or "stencil7" as the block product of every level of the 3-D
    block hierarchies made after the call; returns its return code."""
    if not is_lab():
        raise RuntimeError("the level product is chosen in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_mg3d_multi_level_product(kind if kind is None else kind.encode())


def fused_spmv(op, d_x, d_y, d_partials, cap, count=True):
    """spmv_amd_operator_fused_spmv (LAB build only; include/spmv_amd/lab.h): one fused launch of `op` (an Operator, a pointer to a
    table, or None) on device vectors (objects with .ptr, plain addresses, or None): y = A x and the unreduced partials of x . (A x).
    Returns (return code, number of partials written); count=False passes a null count."""
    if not is_lab():
        raise RuntimeError("spmv_amd_operator_fused_spmv exists in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    used = C.c_int(-1)
    at = lambda v: getattr(v, "ptr", v)  # noqa: E731
    rc = lib().spmv_amd_operator_fused_spmv(getattr(op, "op", op), at(d_x), at(d_y), at(d_partials), int(cap), C.byref(used) if count else None)
    return rc, used.value


def pcg_stage(stage, kind, args, scalars=None):
    """spmv_amd_pcg_stage (LAB build only; include/spmv_amd/lab.h): one stage of the preconditioned solver's own kernels on the
    device data `args` (PcgStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the PCG stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    return lib().spmv_amd_pcg_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(),
                                    None if args is None else C.byref(args), None if scalars is None else C.byref(scalars))


class Comm:
    """Owner of an SpmvAmdComm handle (and of the ctypes callbacks of a staged one)."""

    def __init__(self, handle, keep=()):
        self.handle = handle
        self._keep = keep

    @classmethod
    def rccl(cls, rank, world, id_bytes):
        """RCCL communicator, or None if RCCL could not create it."""
        buf = C.create_string_buffer(bytes(id_bytes), COMM_ID_BYTES)
        h = lib().spmv_amd_comm_create_rccl(rank, world, buf)
        return cls(h) if h else None

    @classmethod
    def staged_over_torch(cls, rank, world, dist):
        """Staged communicator whose host exchange is torch.distributed (CPU tensors, e.g. gloo):
        the transport of the multi-rank tests on a 1-GPU box, and bench.py's way out if RCCL
        cannot be initialised."""
        import torch

        def as_np(ptr, count):
            return np.ctypeslib.as_array(ptr, shape=(count,))

        def halo_cb(user, sp, sn, rp_, rn_, count):
            reqs, prev, nxt = [], None, None
            if rank > 0:
                prev = torch.zeros(count, dtype=torch.float64)
                reqs += [dist.isend(torch.from_numpy(as_np(sp, count).copy()), rank - 1), dist.irecv(prev, rank - 1)]
            if rank < world - 1:
                nxt = torch.zeros(count, dtype=torch.float64)
                reqs += [dist.isend(torch.from_numpy(as_np(sn, count).copy()), rank + 1), dist.irecv(nxt, rank + 1)]
            for r in reqs:
                r.wait()
            if prev is not None:
                as_np(rp_, count)[:] = prev.numpy()
            if nxt is not None:
                as_np(rn_, count)[:] = nxt.numpy()
            return 0

        def allreduce_cb(user, buf, count):
            a = as_np(buf, count)
            t = torch.from_numpy(a.copy())
            dist.all_reduce(t)
            a[:] = t.numpy()
            return 0

        def gather_cb(user, send, n_send, recv, counts, displs):
            mine = torch.from_numpy(as_np(send, n_send).copy())
            if rank == 0:
                out = as_np(recv, sum(counts[r] for r in range(world)))
                out[displs[0]:displs[0] + counts[0]] = mine.numpy()
                for r in range(1, world):
                    t = torch.zeros(counts[r], dtype=torch.float64)
                    dist.recv(t, r)
                    out[displs[r]:displs[r] + counts[r]] = t.numpy()
            else:
                dist.send(mine, 0)
            return 0

        def barrier_cb(user):
            dist.barrier()
            return 0

        return cls.staged(rank, world, halo_cb, allreduce_cb, gather_cb, barrier_cb)

    def selftest(self):
        return lib().spmv_amd_comm_selftest(self.handle)

    def barrier(self):
        return lib().spmv_amd_comm_barrier(self.handle)

    def mailbox_enable(self):
        """Collective: peer-mailbox all-reduce over hipIpc-mapped device memory; True when every rank's passed its self-test."""
        return lib().spmv_amd_comm_mailbox_enable(self.handle) == 1

    def mailbox_prepare(self):
        """Step 1 of the manual set-up: allocate this rank's mailbox, return its 64-byte hipIpc handle (None on failure)."""
        buf = C.create_string_buffer(64)
        return buf.raw if lib().spmv_amd_comm_mailbox_prepare(self.handle, buf) == 0 else None

    def mailbox_connect(self, handles):
        """Step 2: map every rank's mailbox (handles: list of 64-byte blobs in rank order); True on success."""
        blob = b"".join(handles)
        return lib().spmv_amd_comm_mailbox_connect(self.handle, C.create_string_buffer(blob, len(blob)), len(handles)) == 0

    def mailbox_selftest(self, rounds=8):
        """Collective: `rounds` back-to-back mailbox all-reduces with known sums; 0 = all correct."""
        return lib().spmv_amd_comm_mailbox_selftest(self.handle, int(rounds))

    def mailbox_ready(self):
        return lib().spmv_amd_comm_mailbox_ready(self.handle) == 1

    def mailbox_disable(self):
        lib().spmv_amd_comm_mailbox_disable(self.handle)

    def transport(self):
        return lib().spmv_amd_comm_transport(self.handle).decode()

    def transport_ranks(self):
        """Ranks the device transport itself reports (ncclCommCount); 0 for staged / self."""
        return lib().spmv_amd_comm_transport_ranks(self.handle)

    @classmethod
    def staged(cls, rank, world, halo, allreduce, gather=None, barrier=None):
        cbs = (HALO_FN(halo), ALLREDUCE_FN(allreduce), GATHER_FN(gather) if gather else GATHER_FN(), BARRIER_FN(barrier) if barrier else BARRIER_FN())
        h = lib().spmv_amd_comm_create_staged(rank, world, cbs[0], cbs[1], cbs[2], cbs[3], None)
        if not h:
            raise RuntimeError("spmv_amd_comm_create_staged failed")
        return cls(h, cbs)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        lib().spmv_amd_comm_unique_id(buf)
        return buf.raw

    def destroy(self):
        if self.handle:
            lib().spmv_amd_comm_destroy(self.handle)
            self.handle = None


class CgSlab:
    """Resident multi-GPU CG state (spmv_amd_cg_slab_*)."""

    def __init__(self, handle, n_rows):
        if not handle:
            raise RuntimeError("spmv_amd_cg_slab_create failed")
        self.h = handle
        self.n_rows = n_rows
        off, nl, nz = C.c_int(), C.c_int(), C.c_int()
        lib().spmv_amd_cg_slab_info(self.h, C.byref(off), C.byref(nl), C.byref(nz))
        self.row_offset, self.n_local, self.local_nnz = off.value, nl.value, nz.value

    @classmethod
    def from_matrix(cls, host_matrix, comm=None):
        require_gpu()
        return cls(lib().spmv_amd_cg_slab_create(host_matrix.ptr, comm.handle if comm else None), host_matrix.c.rows)

    @classmethod
    def stencil5(cls, n, comm=None):
        require_gpu()
        return cls(lib().spmv_amd_cg_slab_create_stencil5(int(n), comm.handle if comm else None), n * n)

    @classmethod
    def stencil5_as(cls, n, as_rank, as_world, comm):
        """The slab rank `as_rank` of an `as_world`-GPU run would own, on a single self-neighbour rank (LAB build only)."""
        require_gpu()
        if not is_lab():
            raise RuntimeError("stand-in slabs exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        return cls(lib().spmv_amd_cg_slab_create_stencil5_as(int(n), int(as_rank), int(as_world), comm.handle), n * n)

    def set_vectors(self, b=None, x0=None):
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        x0 = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
        lib().spmv_amd_cg_slab_set_vectors(self.h, None if b is None else b.ctypes.data, None if x0 is None else x0.ctypes.data)

    def solve(self, max_iters=1000, tol=1e-6, verbose=0, timers=0):
        cfg = CGConfig(max_iters, tol, verbose, timers)
        st = CGStatsMultiGPU()
        rc = lib().spmv_amd_cg_slab_solve(self.h, C.byref(cfg), C.byref(st))
        if rc != 0:
            raise RuntimeError(f"cg_slab_solve -> {rc}")
        return st

    def history(self, cap=1001):
        h = np.zeros(cap, dtype=np.float64)
        count = lib().spmv_amd_cg_slab_history(self.h, h.ctypes.data, cap)
        return h[: min(count, cap)].copy()

    def gather(self):
        x = np.zeros(self.n_rows, dtype=np.float64)
        lib().spmv_amd_cg_slab_gather(self.h, x.ctypes.data)
        return x

    def spmv(self, x_full):
        x_full = np.ascontiguousarray(x_full, dtype=np.float64)
        y = np.zeros(self.n_local, dtype=np.float64)
        lib().spmv_amd_cg_slab_spmv(self.h, x_full.ctypes.data, y.ctypes.data)
        return y

    def variant(self):
        return lib().spmv_amd_cg_slab_variant(self.h).decode()

    def coefficient_form(self):
        """0: the SpMV streams the CSR values; 1: the symmetric [C, E] + S planes (include/spmv_amd/api.h)."""
        return int(lib().spmv_amd_cg_slab_coefficient_form(self.h))

    def uniform_tiles(self):
        """(uniform, total): the row-lds tiles of the slab's plane-evaluated grid rows that load no coefficient, and all of them."""
        u, t = C.c_longlong(), C.c_longlong()
        lib().spmv_amd_cg_slab_uniform_tiles(self.h, C.byref(u), C.byref(t))
        return int(u.value), int(t.value)

    def tile_classes(self):
        """The tile class map as creation wrote it (LAB build only): uint8 [local grid rows, tiles per grid row], or None."""
        if not is_lab():
            raise RuntimeError("the tile class map is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        count = int(lib().spmv_amd_cg_slab_tile_classes(self.h, None, 0))
        if count == 0:
            return None
        out = np.zeros(count, dtype=np.uint8)
        lib().spmv_amd_cg_slab_tile_classes(self.h, out.ctypes.data, count)
        return out

    def block_map(self, which):
        """The block map of a launch range of the in-loop SpMV (LAB build only): which = 0 the whole slab, 1 the rows that need no
        halo. uint8, one byte per block tile (row blocks x tiles per grid row, flat), 1 = the fast path; None = the range has no map."""
        if not is_lab():
            raise RuntimeError("the block maps are read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        count = int(lib().spmv_amd_cg_slab_block_map(self.h, int(which), None, 0))
        if count == 0:
            return None
        out = np.zeros(count, dtype=np.uint8)
        lib().spmv_amd_cg_slab_block_map(self.h, int(which), out.ctypes.data, count)
        return out

    def slow_blocks(self, which):
        """The slow blocks of a launch range (LAB build only; which as in block_map): int32 indices of the block tiles whose map byte
        is 0, ascending, as the launch behind the direction update inside the block SpMV reads them (empty: none)."""
        if not is_lab():
            raise RuntimeError("the slow-block lists are read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        count = int(lib().spmv_amd_cg_slab_slow_blocks(self.h, int(which), None, 0))
        out = np.zeros(max(count, 0), dtype=np.int32)
        if count > 0:
            lib().spmv_amd_cg_slab_slow_blocks(self.h, int(which), out.ctypes.data, count)
        return out

    def spmv_dot(self):
        """(partials, pAp) the last spmv() in its in-loop form (set_option("spmv_with_dot", 1)) left beside y (LAB build only)."""
        if not is_lab():
            raise RuntimeError("the in-loop SpMV's sum is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        pAp = C.c_double(0.0)
        count = lib().spmv_amd_cg_slab_spmv_dot(self.h, C.byref(pAp), None, 0)
        partials = np.empty(count, dtype=np.float64)
        lib().spmv_amd_cg_slab_spmv_dot(self.h, C.byref(pAp), partials.ctypes.data, count)
        return partials, pAp.value

    def direction_spmv(self, r, p_in, beta, iteration_matches=1, converged=0):
        """spmv_amd_cg_slab_direction_spmv (LAB build only; include/spmv_amd/lab.h): the direction update inside the block SpMV, the
        launch over the slow blocks and the reduction, once, on r and p_in (n_local doubles each). Returns (p_out, Ap, partials, pAp);
        what a launch did not write is NaN."""
        if not is_lab():
            raise RuntimeError("the fused launch alone runs in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        r = np.ascontiguousarray(r, dtype=np.float64)
        p_in = np.ascontiguousarray(p_in, dtype=np.float64)
        p_out, Ap = np.empty_like(r), np.empty_like(r)
        partials = np.empty(len(r), dtype=np.float64)  # more than any plan writes (one per 128 x 1 tile)
        pAp = C.c_double(0.0)
        used = lib().spmv_amd_cg_slab_direction_spmv(self.h, r.ctypes.data, p_in.ctypes.data, float(beta), int(iteration_matches), int(converged),
                                                     p_out.ctypes.data, Ap.ctypes.data, C.byref(pAp), partials.ctypes.data, len(partials))
        if used < 0:
            raise RuntimeError("this slab cannot take the direction update inside the block SpMV (no block map, neighbours, or ring 1)")
        return p_out, Ap, partials[:used], pAp.value

    def initial_form(self):
        """The form the initial stage of a solve would take now (LAB build only; include/spmv_amd/lab.h, spmv_amd_cg_slab_initial_stage):
        bit 0 = no x0 value requested on interior grid rows, bit 1 = r0 stored once, as p0. Nothing is launched."""
        if not is_lab():
            raise RuntimeError("the initial stage's form is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        return int(lib().spmv_amd_cg_slab_initial_stage(self.h, None, None, None, 0, None, None))

    def initial_stage(self):
        """spmv_amd_cg_slab_initial_stage (LAB build only): the first SpMV's launch and the reduction of its partials, once, on the
        stored b and x0. Returns (form, r0, r_vec, partials, rr); r_vec is NaN where the launch did not write."""
        if not is_lab():
            raise RuntimeError("the initial stage alone runs in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        r0, r_vec = np.empty(self.n_local, dtype=np.float64), np.empty(self.n_local, dtype=np.float64)
        partials = np.empty(self.n_local, dtype=np.float64)  # more than any plan writes (one per 128 x 1 tile)
        count, rr = C.c_int(0), C.c_double(0.0)
        form = lib().spmv_amd_cg_slab_initial_stage(self.h, r0.ctypes.data, r_vec.ctypes.data, partials.ctypes.data, len(partials),
                                                    C.byref(count), C.byref(rr))
        if form < 0:
            raise RuntimeError("this slab's first SpMV does not write the residual, or the slab has neighbours")
        return form, r0, r_vec, partials[:count.value], rr.value

    def first_form(self):
        """1 where a solve of at least one iteration would take b itself as p0 and sum b.b in iteration 0's SpMV (LAB build only;
        include/spmv_amd/lab.h, spmv_amd_cg_slab_first_stage), else 0. Nothing is launched."""
        if not is_lab():
            raise RuntimeError("the first stage's form is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        return int(lib().spmv_amd_cg_slab_first_stage(self.h, 0, None, None, None, 0, None, None, None))

    def first_stage(self, reverse=True):
        """spmv_amd_cg_slab_first_stage (LAB build only): iteration 0's block SpMV on the stored b with both partial arrays and both
        reductions, once. Returns (Ap, pAp_partials, bb_partials, rr, pAp); the partial arrays hold the slots the launch writes (one
        per 128 x 1 tile of the slab), NaN where it did not."""
        if not is_lab():
            raise RuntimeError("the first stage alone runs in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        Ap = np.empty(self.n_local, dtype=np.float64)
        pAp_partials, bb_partials = np.empty(self.n_local, dtype=np.float64), np.empty(self.n_local, dtype=np.float64)
        count, rr, pAp = C.c_int(-1), C.c_double(0.0), C.c_double(0.0)
        if lib().spmv_amd_cg_slab_first_stage(self.h, 1 if reverse else 0, Ap.ctypes.data, pAp_partials.ctypes.data, bb_partials.ctypes.data,
                                              len(bb_partials), C.byref(count), C.byref(rr), C.byref(pAp)) != 1:
            raise RuntimeError("a solve on this slab would not take b as p0 now (spmv_amd_cg_slab_first_stage returned 0)")
        return Ap, pAp_partials[:count.value], bb_partials[:count.value], rr.value, pAp.value

    def update_r_stage(self, r, Ap, rr_old, pAp, p_new=None, reverse=False, converged=0):
        """spmv_amd_cg_slab_update_r_stage (LAB build only): the r update of an iteration >= 1, once. p_new None: cg_update_r_kernel on
        (r, Ap); else the launch that recomputes A p' from p_new on the fast row blocks and reads Ap on the slow ones. Returns
        (r_out, partials), NaN where the launch did not write."""
        if not is_lab():
            raise RuntimeError("the r update alone runs in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        r = np.ascontiguousarray(r, dtype=np.float64)
        Ap = np.ascontiguousarray(Ap, dtype=np.float64)
        p_new = None if p_new is None else np.ascontiguousarray(p_new, dtype=np.float64)
        r_out = np.empty_like(r)
        partials = np.empty(len(r) // 128 + 2, dtype=np.float64)
        used = lib().spmv_amd_cg_slab_update_r_stage(self.h, 0 if p_new is None else 1, 1 if reverse else 0, r.ctypes.data,
                                                     None if p_new is None else p_new.ctypes.data, Ap.ctypes.data, float(rr_old), float(pAp),
                                                     int(converged), r_out.ctypes.data, partials.ctypes.data, len(partials))
        if used < 0:
            raise RuntimeError("this slab cannot take the r update that recomputes A p' (a row block that is neither all-fast nor all-slow, ring 1)")
        return r_out, partials[:used]

    def update_r_from_stage(self, src, Ap, rr_old, pAp, recompute=True, reverse=False, converged=0):
        """spmv_amd_cg_slab_update_r_from_stage (LAB build only): iteration 0's r update where r0 and p0 are the one vector src, once.
        recompute False: cg_update_r_from_kernel on (Ap, src); True: the out-of-place instance that recomputes A src on the fast row
        blocks and reads Ap on the slow ones. Returns (r_out, src as it lies on the device afterwards, partials), NaN where the launch
        did not write."""
        if not is_lab():
            raise RuntimeError("the r update alone runs in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        src = np.ascontiguousarray(src, dtype=np.float64)
        Ap = np.ascontiguousarray(Ap, dtype=np.float64)
        r_out, src_back = np.empty_like(src), np.empty_like(src)
        partials = np.empty(len(src) // 128 + 2, dtype=np.float64)
        used = lib().spmv_amd_cg_slab_update_r_from_stage(self.h, 1 if recompute else 0, 1 if reverse else 0, src.ctypes.data, Ap.ctypes.data,
                                                          float(rr_old), float(pAp), int(converged), r_out.ctypes.data, src_back.ctypes.data,
                                                          partials.ctypes.data, len(partials))
        if used < 0:
            raise RuntimeError("this slab cannot take the r update that recomputes A p (a row block that is neither all-fast nor all-slow, ring 1)")
        return r_out, src_back, partials[:used]

    FIRST_FORMS = ("stored", "from b", "from ring slot 0", "in place")

    def first_recompute_form(self):
        """spmv_amd_cg_slab_first_recompute_form (LAB build only): (the form iteration 0 of a solve of at least one iteration would
        take now, the form the last solve's took), each one of FIRST_FORMS: "stored" = A p0 stored and read back, the others = left
        unstored on the fast blocks and recomputed by the r update from b / ring slot 0 / in place on (r, slot 0)."""
        if not is_lab():
            raise RuntimeError("iteration 0's form is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        last = C.c_int(0)
        now = int(lib().spmv_amd_cg_slab_first_recompute_form(self.h, C.byref(last)))
        return self.FIRST_FORMS[now], self.FIRST_FORMS[last.value]

    def ap_form(self):
        """spmv_amd_cg_slab_ap_form (LAB build only): (a solve would recompute A p' in its r update now, the last solve did, the slab's
        block map is eligible, the recomputing launches of the last solve)."""
        if not is_lab():
            raise RuntimeError("the r update's form is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        launches = C.c_int(0)
        bits = int(lib().spmv_amd_cg_slab_ap_form(self.h, C.byref(launches)))
        return bool(bits & 1), bool(bits & 2), bool(bits & 4), launches.value

    @staticmethod
    def workspace_ap_form():
        """ap_form() of the workspace slab cg_solve_device keeps (LAB build only); None: there is no workspace."""
        if not is_lab():
            raise RuntimeError("the r update's form is read through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        launches = C.c_int(0)
        bits = int(lib().spmv_amd_cg_slab_ap_form(None, C.byref(launches)))
        return None if bits < 0 else (bool(bits & 1), bool(bits & 2), bool(bits & 4), launches.value)

    def stored_b(self):
        """The stored right-hand side as it lies on the device now (LAB build only; spmv_amd_cg_slab_stored_b)."""
        if not is_lab():
            raise RuntimeError("the stored right-hand side is read back through the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        b = np.empty(self.n_local, dtype=np.float64)
        lib().spmv_amd_cg_slab_stored_b(self.h, b.ctypes.data)
        return b

    def set_block_rows(self, rows):
        """Grid rows per block tile of the in-loop SpMV (LAB build only): 0 = the one-row kernel, 4 or 8. Rebuilds the block maps."""
        self.set_option("block_rows", rows)

    def loop_shape(self):
        """"single rank[: direction update inside the block SpMV]" | "pipeline ..." | "plain: <who decided>" (include/spmv_amd/api.h)."""
        return lib().spmv_amd_cg_slab_loop_shape(self.h).decode()

    def timeline_solve(self, max_iters=1000, tol=1e-6):
        """One solve with stage-boundary events (no host syncs); returns (stats, {name: value})."""
        lib().spmv_amd_cg_slab_set_timeline(self.h, 1)
        try:
            st = self.solve(max_iters=max_iters, tol=tol)
        finally:
            lib().spmv_amd_cg_slab_set_timeline(self.h, 0)
        names = lib().spmv_amd_cg_slab_timeline_names().decode().split(",")
        v = np.zeros(len(names), dtype=np.float64)
        count = lib().spmv_amd_cg_slab_timeline(self.h, v.ctypes.data, len(v))
        return st, ({k: float(x) for k, x in zip(names, v)} if count == len(names) else {})

    def placement(self):
        """What the placement of the coefficient stream at creation did, or None if it did not run."""
        v = (C.c_double * 4)()
        lib().spmv_amd_cg_slab_placement.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        if lib().spmv_amd_cg_slab_placement(self.h, v, 4) != 4:
            return None
        return {"kind": "coefficient candidates", "candidates": int(v[1]), "spmv_ms_before": float(v[2]), "spmv_ms_kept": float(v[3])}

    def setup_ms(self):
        """Wall ms of creation's set-up phases (outside every timed region)."""
        v = (C.c_double * 5)()
        lib().spmv_amd_cg_slab_setup_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib().spmv_amd_cg_slab_setup_ms(self.h, v, 5)
        return dict(zip(("matrix_to_hbm", "streams_and_vectors", "verify_and_plans", "coefficient_placement", "tile_runs"), (float(x) for x in v)))

    def tile_runs(self):
        """Row-lds tiles per XCD and run as tuned at creation, or None if the trial did not run."""
        v = (C.c_double * 4)()
        lib().spmv_amd_cg_slab_tile_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        if lib().spmv_amd_cg_slab_tile_runs(self.h, v, 4) != 4:
            return None
        return {"rule": int(v[0]), "kept": int(v[1]), "spmv_ms_rule": float(v[2]), "spmv_ms_kept": float(v[3])}

    def spmv_launch_ms(self):
        """The timed in-loop SpMV launches of the last solve, one by one (ms)."""
        out = (C.c_float * 1024)()
        lib().spmv_amd_cg_slab_spmv_launch_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        count = lib().spmv_amd_cg_slab_spmv_launch_ms(self.h, out, 1024)
        return np.array(out[:min(count, 1024)], dtype=np.float64)

    def set_option(self, name, value):
        """Option of this slab (LAB build only; include/spmv_amd/lab.h lists them): A/B runs on the same allocations."""
        if not is_lab():
            raise RuntimeError("slab options exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
        if lib().spmv_amd_cg_slab_set_option(self.h, name.encode(), int(value)) != 0:
            raise ValueError(f"unknown slab option {name!r}")

    def time_spmv(self, reps):
        ms = (C.c_float * reps)()
        lib().spmv_amd_cg_slab_time_spmv(self.h, reps, ms)
        return np.array(ms[:], dtype=np.float64)

    def destroy(self):
        if self.h:
            lib().spmv_amd_cg_slab_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- BiCGSTAB (include/spmv_amd/api.h; csrc/bicgstab.hip)
class BicgstabScalars(C.Structure):
    """SpmvAmdBicgstabScalars (include/spmv_amd/lab.h): the device scalars of one BiCGSTAB solve."""
    _fields_ = [("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double), ("omega", C.c_double), ("beta", C.c_double),
                ("b_norm", C.c_double), ("residual", C.c_double), ("s_norm", C.c_double), ("iterations", C.c_int), ("converged", C.c_int),
                ("breakdown", C.c_int), ("x_step", C.c_int), ("stop", C.c_int), ("pad", C.c_int)]


class BicgstabStageArgs(C.Structure):
    """SpmvAmdBicgstabStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_bicgstab_stage call."""
    _fields_ = [("n", C.c_size_t), ("b", C.c_void_p), ("dinv", C.c_void_p), ("x", C.c_void_p), ("r", C.c_void_p), ("rhat", C.c_void_p),
                ("p", C.c_void_p), ("phat", C.c_void_p), ("shat", C.c_void_p), ("v", C.c_void_p), ("t", C.c_void_p),
                ("partials", C.c_void_p), ("count", C.c_int), ("which", C.c_int), ("tol", C.c_double), ("hist", C.c_void_p),
                ("hist_cap", C.c_int)]


def bicgstab_solve(op, host_matrix, precond, b, x0, tol=1e-6, max_iters=1000, verbose=0, timers=0):
    """spmv_amd_bicgstab_solve_device; returns x, history, stats like pcg_solve_device (raises RuntimeError on a refusal)."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    cfg = CGConfig(max_iters, tol, verbose, timers)
    st = CGStats()
    L = _pcg_lib()
    L.spmv_amd_bicgstab_solve_device.argtypes = L.spmv_amd_pcg_solve_device.argtypes
    L.spmv_amd_bicgstab_last_history.argtypes = [C.c_void_p, C.c_int]
    rc = L.spmv_amd_bicgstab_solve_device(op.op, host_matrix.ptr, precond.handle, b.ctypes.data, x.ctypes.data, C.byref(cfg), C.byref(st))
    if rc != 0:
        raise RuntimeError(f"bicgstab_solve_device -> {rc}")
    hist = np.zeros(max_iters + 1, dtype=np.float64)
    count = L.spmv_amd_bicgstab_last_history(hist.ctypes.data, len(hist))
    return x, hist[:count].copy(), st


def bicgstab_stage(stage, kind, args, scalars=None):
    """spmv_amd_bicgstab_stage (LAB build only; include/spmv_amd/lab.h): one stage of the BiCGSTAB solver's own kernels on the
    device data `args` (BicgstabStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the BiCGSTAB stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    L = lib()
    L.spmv_amd_bicgstab_stage.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(BicgstabStageArgs), C.POINTER(BicgstabScalars)]
    L.spmv_amd_bicgstab_stage.restype = C.c_int
    return L.spmv_amd_bicgstab_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(),
                                     None if args is None else C.byref(args), None if scalars is None else C.byref(scalars))


# ---------------------------------------------------------------- batched BiCGSTAB (include/spmv_amd/api.h; csrc/bicgstab_multi.hip)
class BicgstabMultiColumn(C.Structure):
    """SpmvAmdBicgstabMultiColumn (include/spmv_amd/lab.h): the per-column state of a batched BiCGSTAB solve."""
    _fields_ = [("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double), ("omega", C.c_double), ("beta", C.c_double),
                ("b_norm", C.c_double), ("residual", C.c_double), ("s_norm", C.c_double), ("active", C.c_int), ("done", C.c_int),
                ("iterations", C.c_int), ("converged", C.c_int), ("breakdown", C.c_int), ("x_step", C.c_int), ("pad", C.c_int * 2)]


class BicgstabMultiStageArgs(C.Structure):
    """SpmvAmdBicgstabMultiStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_bicgstab_multi_stage call."""
    _fields_ = [("n", C.c_size_t), ("X", C.c_void_p), ("R", C.c_void_p), ("RH", C.c_void_p), ("P", C.c_void_p), ("PH", C.c_void_p),
                ("SH", C.c_void_p), ("V", C.c_void_p), ("T", C.c_void_p), ("dinv", C.c_void_p), ("cols", C.c_void_p),
                ("partials", C.c_void_p), ("count", C.c_longlong), ("which", C.c_int), ("tol", C.c_double), ("hist", C.c_void_p),
                ("hist_cap", C.c_int)]


def _bicgstab_multi_lib():
    L = _pcg_lib()
    if not getattr(L, "_bicgstab_multi_sigs", False):
        L.spmv_amd_bicgstab_solve_device_multi.argtypes = L.spmv_amd_pcg_solve_device_multi.argtypes
        L.spmv_amd_bicgstab_last_history_multi.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.spmv_amd_bicgstab_multi_workspace_bytes.argtypes = []
        L.spmv_amd_bicgstab_multi_workspace_bytes.restype = C.c_size_t
        L._bicgstab_multi_sigs = True
    return L


def bicgstab_solve_multi(op, host_matrix, precond, Bk, X0k, tol=1e-6, max_iters=1000, verbose=0, timers=0):
    """spmv_amd_bicgstab_solve_device_multi: k independent BiCGSTAB solves sharing the SpMM. Bk, X0k: (k, n).
    Returns X (k, n), a list of k residual histories and a list of k CGStats like pcg_solve_multi (raises RuntimeError on a refusal)."""
    Bk = np.ascontiguousarray(np.atleast_2d(Bk), dtype=np.float64)
    X = np.ascontiguousarray(np.atleast_2d(X0k), dtype=np.float64).copy()
    k = Bk.shape[0]
    assert X.shape == Bk.shape
    cfg = CGConfig(max_iters, tol, verbose, timers)
    stats = (CGStats * k)()
    L = _bicgstab_multi_lib()
    rc = L.spmv_amd_bicgstab_solve_device_multi(op.op, host_matrix.ptr, precond.handle, k, Bk.ctypes.data, X.ctypes.data, C.byref(cfg), stats)
    if rc != 0:
        raise RuntimeError(f"bicgstab_solve_device_multi -> {rc}")
    hists = []
    for j in range(k):
        h = np.zeros(max_iters + 1, dtype=np.float64)
        count = L.spmv_amd_bicgstab_last_history_multi(j, h.ctypes.data, len(h))
        hists.append(h[:count].copy())
    return X, hists, list(stats)


def bicgstab_multi_workspace_bytes():
    """spmv_amd_bicgstab_multi_workspace_bytes: device bytes the batched BiCGSTAB workspace holds now."""
    return int(_bicgstab_multi_lib().spmv_amd_bicgstab_multi_workspace_bytes())


def bicgstab_multi_stage(stage, kind, k, args):
    """spmv_amd_bicgstab_multi_stage (LAB build only; include/spmv_amd/lab.h): one stage of the batched BiCGSTAB solver's own kernels
    on the device data `args` (BicgstabMultiStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched-BiCGSTAB stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    L = lib()
    L.spmv_amd_bicgstab_multi_stage.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(BicgstabMultiStageArgs)]
    L.spmv_amd_bicgstab_multi_stage.restype = C.c_int
    return L.spmv_amd_bicgstab_multi_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(), int(k),
                                           None if args is None else C.byref(args))


# ---------------------------------------------------------------- GCR(m) (include/spmv_amd/api.h; csrc/gcr.hip)
GCR_MAX_RESTART = 32
GCR_DOT_CHUNK = 8    # SPMV_AMD_GCR_DOT_CHUNK (include/spmv_amd/lab.h)
GCR_ORTH_CHUNK = 4   # SPMV_AMD_GCR_ORTH_CHUNK


class GcrScalars(C.Structure):
    """SpmvAmdGcrScalars (include/spmv_amd/lab.h): the device scalars of one GCR solve."""
    _fields_ = [("gamma", C.c_double * GCR_MAX_RESTART), ("beta", C.c_double * GCR_MAX_RESTART), ("alpha", C.c_double), ("rho", C.c_double),
                ("b_norm", C.c_double), ("residual", C.c_double), ("iterations", C.c_int), ("converged", C.c_int), ("breakdown", C.c_int),
                ("stop", C.c_int)]


class GcrStageArgs(C.Structure):
    """SpmvAmdGcrStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_gcr_stage call."""
    _fields_ = [("n", C.c_size_t), ("b", C.c_void_p), ("v", C.c_void_p), ("dinv", C.c_void_p), ("x", C.c_void_p), ("r", C.c_void_p),
                ("zs", C.c_void_p), ("z_in", C.c_void_p), ("Q", C.POINTER(C.c_void_p)), ("Z", C.POINTER(C.c_void_p)), ("slot", C.c_int),
                ("partials", C.c_void_p), ("count", C.c_int), ("which", C.c_int), ("tol", C.c_double), ("hist", C.c_void_p),
                ("hist_cap", C.c_int)]


def _gcr_lib():
    L = _pcg_lib()
    if not getattr(L, "_gcr_sigs", False):
        L.spmv_amd_gcr_solve_device.argtypes = [C.POINTER(SpmvOperator), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.POINTER(CGConfig), C.POINTER(CGStats)]
        L.spmv_amd_gcr_last_history.argtypes = [C.c_void_p, C.c_int]
        L.spmv_amd_gcr_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_char_p]
        L.spmv_amd_gcr_workspace_bytes.restype = C.c_size_t
        L._gcr_sigs = True
    return L


def gcr_solve(op, host_matrix, precond, b, x0, restart=0, tol=1e-6, max_iters=1000, verbose=0, timers=0):
    """spmv_amd_gcr_solve_device; returns x, history, stats like bicgstab_solve (raises RuntimeError on a refusal)."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    cfg = CGConfig(max_iters, tol, verbose, timers)
    st = CGStats()
    L = _gcr_lib()
    rc = L.spmv_amd_gcr_solve_device(op.op, host_matrix.ptr, precond.handle, restart, b.ctypes.data, x.ctypes.data, C.byref(cfg), C.byref(st))
    if rc != 0:
        raise RuntimeError(f"gcr_solve_device -> {rc}")
    hist = np.zeros(max_iters + 1, dtype=np.float64)
    count = L.spmv_amd_gcr_last_history(hist.ctypes.data, len(hist))
    return x, hist[:count].copy(), st


def gcr_workspace_bytes(rows, restart, kind):
    """spmv_amd_gcr_workspace_bytes: 0 for refused arguments."""
    return int(_gcr_lib().spmv_amd_gcr_workspace_bytes(rows, restart, kind if kind is None else kind.encode()))


def gcr_stage(stage, kind, args, scalars=None):
    """spmv_amd_gcr_stage (LAB build only; include/spmv_amd/lab.h): one stage of the GCR solver's own kernels on the device data
    `args` (GcrStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the GCR stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    L = lib()
    L.spmv_amd_gcr_stage.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(GcrStageArgs), C.POINTER(GcrScalars)]
    L.spmv_amd_gcr_stage.restype = C.c_int
    return L.spmv_amd_gcr_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(),
                                None if args is None else C.byref(args), None if scalars is None else C.byref(scalars))


# ---------------------------------------------------------------- batched GCR(m) (include/spmv_amd/api.h; csrc/gcr_multi.hip)
GCR_MULTI_DOT_CHUNK = 4    # SPMV_AMD_GCR_MULTI_DOT_CHUNK (include/spmv_amd/lab.h)
GCR_MULTI_ORTH_CHUNK = 2   # SPMV_AMD_GCR_MULTI_ORTH_CHUNK


class GcrMultiColumn(C.Structure):
    """SpmvAmdGcrMultiColumn (include/spmv_amd/lab.h): the per-column state of a batched GCR solve."""
    _fields_ = [("gamma", C.c_double * GCR_MAX_RESTART), ("beta", C.c_double * GCR_MAX_RESTART), ("alpha", C.c_double), ("rho", C.c_double),
                ("b_norm", C.c_double), ("residual", C.c_double), ("done", C.c_int), ("iterations", C.c_int), ("converged", C.c_int),
                ("breakdown", C.c_int)]


class GcrMultiStageArgs(C.Structure):
    """SpmvAmdGcrMultiStageArgs (include/spmv_amd/lab.h): device pointers and sizes of one spmv_amd_gcr_multi_stage call."""
    _fields_ = [("n", C.c_size_t), ("X", C.c_void_p), ("R", C.c_void_p), ("AX", C.c_void_p), ("z_in", C.c_void_p), ("ZS", C.c_void_p),
                ("Q", C.POINTER(C.c_void_p)), ("Z", C.POINTER(C.c_void_p)), ("slot", C.c_int), ("dinv", C.c_void_p), ("cols", C.c_void_p),
                ("shadow", C.c_void_p), ("partials", C.c_void_p), ("count", C.c_longlong), ("which", C.c_int), ("tol", C.c_double),
                ("hist", C.c_void_p), ("hist_cap", C.c_int)]


def _gcr_multi_lib():
    L = _pcg_lib()
    if not getattr(L, "_gcr_multi_sigs", False):
        L.spmv_amd_gcr_solve_device_multi.argtypes = [C.POINTER(SpmvOperator), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.POINTER(CGConfig), C.POINTER(CGStats)]
        L.spmv_amd_gcr_last_history_multi.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.spmv_amd_gcr_multi_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p]
        L.spmv_amd_gcr_multi_workspace_bytes.restype = C.c_size_t
        L._gcr_multi_sigs = True
    return L


def gcr_solve_multi(op, host_matrix, precond, Bk, X0k, restart=0, tol=1e-6, max_iters=1000, verbose=0, timers=0):
    """spmv_amd_gcr_solve_device_multi: k independent GCR(restart) solves sharing the SpMM and the preconditioner's block application.
    Bk, X0k: (k, n). Returns X (k, n), a list of k residual histories and a list of k CGStats like bicgstab_solve_multi (raises
    RuntimeError on a refusal)."""
    Bk = np.ascontiguousarray(np.atleast_2d(Bk), dtype=np.float64)
    X = np.ascontiguousarray(np.atleast_2d(X0k), dtype=np.float64).copy()
    k = Bk.shape[0]
    assert X.shape == Bk.shape
    cfg = CGConfig(max_iters, tol, verbose, timers)
    stats = (CGStats * max(k, 1))()
    L = _gcr_multi_lib()
    rc = L.spmv_amd_gcr_solve_device_multi(op.op, host_matrix.ptr, precond.handle, restart, k, Bk.ctypes.data, X.ctypes.data, C.byref(cfg), stats)
    if rc != 0:
        raise RuntimeError(f"gcr_solve_device_multi -> {rc}")
    hists = []
    for j in range(k):
        h = np.zeros(max_iters + 1, dtype=np.float64)
        count = L.spmv_amd_gcr_last_history_multi(j, h.ctypes.data, len(h))
        hists.append(h[:count].copy())
    return X, hists, list(stats)[:k]


def gcr_multi_workspace_bytes(rows, nrhs, restart, kind):
    """spmv_amd_gcr_multi_workspace_bytes: 0 for refused arguments."""
    return int(_gcr_multi_lib().spmv_amd_gcr_multi_workspace_bytes(rows, nrhs, restart, kind if kind is None else kind.encode()))


def gcr_multi_stage(stage, kind, k, args):
    """spmv_amd_gcr_multi_stage (LAB build only; include/spmv_amd/lab.h): one stage of the batched GCR solver's own kernels on the
    device data `args` (GcrMultiStageArgs) points to; returns its return code (0, or non-zero for a refusal)."""
    if not is_lab():
        raise RuntimeError("the batched-GCR stages exist in the LAB build only (binding.use_lab(), lib/libspmv_amd_lab.so)")
    L = lib()
    L.spmv_amd_gcr_multi_stage.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(GcrMultiStageArgs)]
    L.spmv_amd_gcr_multi_stage.restype = C.c_int
    return L.spmv_amd_gcr_multi_stage(stage if stage is None else stage.encode(), kind if kind is None else kind.encode(), int(k),
                                      None if args is None else C.byref(args))
