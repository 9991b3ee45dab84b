// cg_device.hip -- the reference-named entry points on the slab solver (cg_slab.hpp): cg_solve_device on a borrowed operator
// (reference src/solvers/cg_solver.cu:436-706; cg_single.hip calls cg_solve_on_operator) with the workspace it keeps between
// calls, and cg_solve_mgpu_partitioned (src/solvers/cg_solver_mgpu_partitioned.cu:236-908).
#include <atomic>
#include <mutex>
#include <thread>

#include "cg_slab.hpp"

namespace {
SpmvAmdCgSlab* g_workspace = nullptr;  // vectors, direction ring, scalars of cg_solve_device, kept between calls
int g_workspace_device = -1;
// one solve at a time on the shared workspace (the reference's operators are not re-entrant either, SURVEY 8b "Threading";
// two host threads calling cg_solve_device are serialised here instead of racing on the buffers)
std::mutex g_workspace_lock;
// The thread inside cg_solve_on_operator (it holds the lock for the whole solve, callbacks into a foreign run_device included).
// A release asked for BY THAT THREAD -- a caller's run_device that calls spmv_amd_cg_release_workspace() or an operator's
// free() -- cannot take the lock again and must not pull the vectors from under the running loop: it is noted and carried
// out when the solve returns.
std::atomic<std::thread::id> g_workspace_owner{std::thread::id()};  // read without the lock by release_cg_workspace() on any thread
bool g_release_pending = false;  // only ever touched by the owner thread (which holds the lock)
void release_cg_workspace_locked() {
    spmv_amd::release_cg_multi_workspace_locked();  // the batched solver's (cg_multi.hip) lives and goes with this one
    spmv_amd::release_pcg_workspace_locked();       // and the preconditioned solver's (pcg.hip)
    spmv_amd::release_pcg_multi_workspace_locked();  // and the batched preconditioned solver's (pcg_multi.hip)
    spmv_amd::release_bicgstab_workspace_locked();   // and the BiCGSTAB solver's (bicgstab.hip)
    spmv_amd::release_gcr_workspace_locked();        // and the GCR solver's (gcr.hip)
    spmv_amd::release_bicgstab_multi_workspace_locked();  // and the batched BiCGSTAB solver's (bicgstab_multi.hip)
    spmv_amd::release_gcr_multi_workspace_locked();       // and the batched GCR solver's (gcr_multi.hip)
    if (g_workspace == nullptr) return;
    spmv_amd_cg_slab_destroy(g_workspace);
    g_workspace = nullptr;
}
}  // namespace

namespace spmv_amd {

void release_cg_workspace() {
    if (g_workspace_owner.load(std::memory_order_acquire) == std::this_thread::get_id()) {  // only ever equal on the thread that set it
        g_release_pending = true;
        return;
    }
    std::lock_guard<std::mutex> guard(g_workspace_lock);
    release_cg_workspace_locked();
}

#ifdef SPMV_AMD_LAB
// the workspace slab of cg_solve_device as it stands (null: none), for the LAB build's hooks that report on the last solve
const SpmvAmdCgSlab* cg_workspace_slab() {
    std::lock_guard<std::mutex> guard(g_workspace_lock);
    return g_workspace;
}
#endif

// The lock and the owner rule of every solve on the workspaces: cg_solve_on_operator below, the batched solve (cg_multi.hip).
CgWorkspaceScope::CgWorkspaceScope() {
    g_workspace_lock.lock();
    g_release_pending = false;
    g_workspace_owner.store(std::this_thread::get_id(), std::memory_order_release);
}

CgWorkspaceScope::~CgWorkspaceScope() {
    g_workspace_owner.store(std::thread::id(), std::memory_order_release);
    if (g_release_pending) release_cg_workspace_locked();
    g_release_pending = false;
    g_workspace_lock.unlock();
}

// The loop of spmv_amd_cg_slab_solve driven through the caller's operator: the same fused kernels, direction ring,
// deferred x update, status record in host-coherent memory (no blocking read-back per iteration, no event pairs unless
// detailed timers ask for them), one rank, default stream. What stays the reference's: run_device(d_x, d_y) is the only
// thing asked of an operator this library does not own; b / x are host arrays, uploaded before and downloaded after the
// timed region (:458-474, :646-649); ||r0|| is the stopping test's denominator; the direction update is rounded as
// update_p_kernel rounds it. The reference allocates and frees its vectors in every call; here they are kept until an
// operator's free() (the harness solves the same system 13 times: 3 warm-ups + 10 runs, src/main/cg_solver.cu:154-178).
int cg_solve_on_operator(SpmvOperator* op, int n, const double* b, double* x, const CGConfig& config, CGStats* stats,
                         std::vector<double>* history) {
    CgWorkspaceScope scope;  // the lock, and this thread marked as the one inside the solve: a release it asks for meanwhile is carried out on the way out
    int device = 0;
    HIP_CHECK(hipGetDevice(&device));
    if (g_workspace != nullptr && (g_workspace->n != n || g_workspace_device != device)) release_cg_workspace_locked();
    if (g_workspace == nullptr) {
        SpmvAmdCgSlab* s = new SpmvAmdCgSlab();
        s->comm = self_comm();
        s->op = op;
        s->n = s->n_local = n;
        s->grid = -1;
        s->label = "CG-DEVICE";
        s->device_form = true;
        make_common(s);
        g_workspace = s;
        g_workspace_device = device;
    } else {
        adopt_operator(g_workspace, op);
    }
    SpmvAmdCgSlab* s = g_workspace;
    upload(s->b, b, (size_t)n);
    upload(s->x0, x, (size_t)n);
    s->x0_known_zero = false;
    const CGConfigMultiGPU cfg = {config.max_iters, config.tolerance, config.verbose, config.enable_detailed_timers};
    CGStatsMultiGPU st;
    if (spmv_amd_cg_slab_solve(s, &cfg, &st) != 0) return 1;
    download(x, s->x, (size_t)n);
    *history = s->history;
    // ||r0|| and the last residual copied back are the history's ends; the slab's six timers onto the reference's four
    const double r0 = s->history.empty() ? 0.0 : s->history.front();
    const double last = st.converged ? st.residual_norm : (s->history.empty() ? 0.0 : s->history.back());
    fill_device_stats(stats, st.iterations, st.converged != 0, last, r0, config, st.time_total_ms,
                      st.time_spmv_ms + (config.enable_detailed_timers ? st.time_initial_r_ms : 0.0), st.time_blas1_ms,
                      st.time_reductions_ms + st.time_dot_rs_initial_ms);
    return 0;
}

}  // namespace spmv_amd

// ---- reference entry point ----
int cg_solve_mgpu_partitioned(SpmvOperator* spmv_op, MatrixData* mat, const double* b, double* x,
                              CGConfigMultiGPU config, CGStatsMultiGPU* stats) {
    (void)spmv_op;  // unused upstream as well; callers pass NULL
    SpmvAmdComm* comm = world_comm();
    const int rank = comm->rank, world = comm->world;
    if (rank == 0 && config.verbose >= 1) {
        printf("\n========================================\n");
        printf("Multi-GPU CG Solver (PARTITIONED CSR)\n");
        printf("========================================\n");
        printf("Ranks: %d (transport: %s)\n", world, comm->transport());
        printf("Problem size: %d unknowns\n", mat->rows);
        printf("Max iterations: %d\n", config.max_iters);
        printf("Tolerance: %.1e\n", config.tolerance);
        printf("========================================\n\n");
    }
    SpmvAmdCgSlab* s = create_from_matrix(mat, comm, /*setup_trials=*/false);  // one solve, then destroyed: no timed trials
    if (!s) return 1;
    if (config.verbose >= 1)
        printf("[Rank %d] Rows: [%d:%d) (%d rows), local nnz %lld\n", rank, s->row_offset,
               s->row_offset + s->n_local, s->n_local, s->A.view.nnz_local);
    spmv_amd_cg_slab_set_vectors(s, b, x);
    spmv_amd_cg_slab_solve(s, &config, stats);

    // slowest rank decides the wall time (reference :748-800 reduces six timers with MPI_MAX)
    if (world > 1) {
        // max over ranks through a sum of one-hot slots would need P slots; the timers only feed
        // rank 0's report, so gather them with the collective we have: all-reduce of per-rank slots.
        std::vector<double> slots((size_t)world * 6, 0.0);
        double mine[6] = {stats->time_total_ms,       stats->time_spmv_ms,      stats->time_blas1_ms,
                          stats->time_reductions_ms, stats->time_allreduce_ms, stats->time_allgather_ms};
        memcpy(&slots[(size_t)rank * 6], mine, sizeof mine);
        double* d_slots = device_alloc<double>(slots.size());
        upload(d_slots, slots.data(), slots.size());
        {
            WatchdogScope guard("all-reduce of the ranks' timers", rank, -1, report_slab_state, s);
            comm->allreduce_sum(d_slots, (int)slots.size(), s->compute);
            HIP_CHECK(hipStreamSynchronize(s->compute));
        }
        download(slots.data(), d_slots, slots.size());
        device_release(d_slots);
        if (rank == 0) {
            double mx[6], mn[6];
            for (int k = 0; k < 6; ++k) {
                mx[k] = mn[k] = slots[k];
                for (int r = 1; r < world; ++r) {
                    const double v = slots[(size_t)r * 6 + k];
                    mx[k] = v > mx[k] ? v : mx[k];
                    mn[k] = v < mn[k] ? v : mn[k];
                }
            }
            stats->time_total_ms = mx[0];
            stats->time_spmv_ms = mx[1];
            stats->time_blas1_ms = mx[2];
            stats->time_reductions_ms = mx[3];
            stats->time_allreduce_ms = mx[4];
            stats->time_allgather_ms = mx[5];
            printf("Total time: %.2f ms (max), %.2f ms (min) - Load imbalance: %.1f%%\n", mx[0], mn[0],
                   100.0 * (mx[0] - mn[0]) / mx[0]);
        }
    } else if (rank == 0 && config.verbose >= 1) {
        printf("Total time: %.2f ms\n", stats->time_total_ms);
    }

    spmv_amd_cg_slab_gather(s, x);
    if (rank == 0) solution_checksums(x, mat->rows, &stats->solution_sum, &stats->solution_norm);
    spmv_amd_cg_slab_destroy(s);
    return 0;
}

// Frees what cg_solve_device keeps between calls (five vectors + the direction ring). A caller that drives its OWN operator
// table through cg_solve_device never passes through this library's operator free(), which is where the workspace is
// otherwise released.
extern "C" void spmv_amd_cg_release_workspace(void) { spmv_amd::release_cg_workspace(); }

extern "C" int spmv_amd_cg_solve_mgpu_partitioned(MatrixData* mat, const double* b, double* x, const CGConfigMultiGPU* config,
                                                  CGStatsMultiGPU* stats) {
    return cg_solve_mgpu_partitioned(nullptr, mat, b, x, *config, stats);
}
