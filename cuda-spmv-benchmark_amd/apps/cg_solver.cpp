// cg_solver -- counterpart of reference src/main/cg_solver.cu: b = 1, x0 = 0, 3 warm-up solves,
// then 10 timed solves from x0 = 0 each.
//   cg_solver <matrix.mtx | --stencil=N> [--mode=<m1,..>] [--host|--device] [--tol=1e-6]
//             [--maxiter=1000] [--timers] [--json=<file>] [--csv=<file>] [--precond=none|jacobi|chebyshev[:K]|multigrid[:NU]|amg[:NU]]
//             [--solver=cg|bicgstab|gcr[:M]]
// --precond runs the preconditioned solver (spmv_amd_pcg_solve_device, device only); its JSON / CSV carry the mode string
// <operator>+<kind>. Without it the binary takes cg_solve_device / cg_solve as before. chebyshev = the polynomial preconditioner
// of degree 4, chebyshev:K of degree K (0..32), both on the automatic interval; the mode string is <operator>+chebyshev<K>.
// multigrid = the aggregation multigrid V(1, 1) cycle (stencil5-csr, and stencil7-csr through the 3-D creator), multigrid:NU the V(NU, NU) cycle (0..8); the mode string is
// <operator>+multigrid<NU>. amg[:NU] = the aggregation AMG V(NU, NU) cycle (default 1, strength 0.08) made from the matrix itself, on
// --mode=cusparse-csr only: any matrix the general CSR operator holds; the mode string is cusparse-csr+amg<NU>.
// --solver=bicgstab runs spmv_amd_bicgstab_solve_device (nonsymmetric matrices; device only) with --precond=none (the default) or
// jacobi; the mode string is <operator>+bicgstab or <operator>+jacobi+bicgstab. --solver=cg (the default) is everything above.
// --solver=gcr[:M] runs spmv_amd_gcr_solve_device (nonsymmetric matrices; device only), restarted every M = 1..32 iterations (gcr: the
// default, 16), with every --precond value --solver=cg takes (none is the default); the mode string is <operator>+gcr<M> or
// <operator>+<kind as above>+gcr<M>.
// (The reference's own main, unmodified, also builds against this library: INTEGRATION.md. Unlike
// it, this binary restarts every timed solve from x0 = 0 instead of from the warm-up's solution.)
#include <algorithm>
#include <cmath>

#include "app_common.hpp"

namespace {
// num_runs preconditioned solves from x0 = 0 with the harness's statistics rule (csrc/harness.hip): mean and population sigma,
// runs further than 2 sigma from the mean dropped, then median / min / max of the survivors; the stats of the last run.
typedef int (*PrecondSolve)(SpmvOperator*, MatrixData*, const SpmvAmdPrecond*, const double*, double*, const CGConfig*, CGStats*);
int pcg_runs(SpmvOperator* op, MatrixData* mat, const SpmvAmdPrecond* m, const double* b, std::vector<double>& x, CGConfig cfg,
             int num_runs, BenchmarkStats* bs, CGStats* st, PrecondSolve solve = spmv_amd_pcg_solve_device, int gcr_restart = 0) {
    std::vector<double> t;
    for (int k = 0; k < num_runs; ++k) {
        std::fill(x.begin(), x.end(), 0.0);
        // gcr_restart > 0: the GCR solver, which takes its restart beside the common arguments
        if ((gcr_restart > 0 ? spmv_amd_gcr_solve_device(op, mat, m, gcr_restart, b, x.data(), &cfg, st) : solve(op, mat, m, b, x.data(), &cfg, st)) != 0)
            return 1;
        t.push_back(st->time_total_ms);
    }
    double mean = 0.0, q = 0.0;
    for (double v : t) mean += v;
    mean /= (double)t.size();
    for (double v : t) q += (v - mean) * (v - mean);
    const double sigma = std::sqrt(q / (double)t.size());
    std::vector<double> keep;
    for (double v : t)
        if (sigma == 0.0 || std::fabs(v - mean) <= 2.0 * sigma) keep.push_back(v);
    std::sort(keep.begin(), keep.end());
    double km = 0.0, kq = 0.0;
    for (double v : keep) km += v;
    km /= (double)keep.size();
    for (double v : keep) kq += (v - km) * (v - km);
    bs->mean_ms = km;
    bs->std_dev_ms = std::sqrt(kq / (double)keep.size());
    bs->median_ms = keep[keep.size() / 2];
    bs->min_ms = keep.front();
    bs->max_ms = keep.back();
    bs->valid_runs = (int)keep.size();
    bs->outliers_removed = (int)(t.size() - keep.size());
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const char *matrix = nullptr, *modes_text = nullptr, *json = nullptr, *csv = nullptr, *precond = nullptr, *solver = "cg";
    int stencil = 0, stencil3d = 0, maxiter = 1000, timers = 0;
    bool device = true;
    double tol = 1e-6;
    for (int i = 1; i < argc; ++i) {
        if (const char* v = app::value_of(argv[i], "--mode=")) modes_text = v;
        else if (const char* v2 = app::value_of(argv[i], "--json=")) json = v2;
        else if (const char* v3 = app::value_of(argv[i], "--csv=")) csv = v3;
        else if (const char* v4 = app::value_of(argv[i], "--stencil=")) stencil = atoi(v4);
        else if (const char* v8 = app::value_of(argv[i], "--stencil3d=")) stencil3d = atoi(v8);
        else if (const char* v5 = app::value_of(argv[i], "--tol=")) tol = atof(v5);
        else if (const char* v6 = app::value_of(argv[i], "--maxiter=")) maxiter = atoi(v6);
        else if (const char* v7 = app::value_of(argv[i], "--precond=")) precond = v7;
        else if (const char* v9 = app::value_of(argv[i], "--solver=")) solver = v9;
        else if (!strcmp(argv[i], "--host")) device = false;
        else if (!strcmp(argv[i], "--device")) device = true;
        else if (!strcmp(argv[i], "--timers")) timers = 1;
        else if (argv[i][0] != '-') matrix = argv[i];
    }
    if (modes_text == nullptr) modes_text = stencil3d > 0 ? "stencil7-csr" : "stencil5-csr";  // the grid's own operator
    if (!matrix && stencil <= 0 && stencil3d <= 0) {
        fprintf(stderr, "Usage: %s <matrix.mtx | --stencil=N | --stencil3d=N> [--mode=<modes>] [--host|--device] [--tol=] [--maxiter=] [--timers] [--json=] [--csv=]\n", argv[0]);
        return 1;
    }
    int gcr = 0;  // > 0: --solver=gcr[:M], the restart
    if (!strncmp(solver, "gcr", 3) && (solver[3] == '\0' || solver[3] == ':')) {
        char* end = nullptr;
        const long k = solver[3] == ':' ? strtol(solver + 4, &end, 10) : 16;
        if (solver[3] == ':' && (end == solver + 4 || *end != '\0' || k < 1 || k > 32)) {
            fprintf(stderr, "Error: --solver=gcr:M takes a restart M of 1..32, not '%s'\n", solver + 4);
            return 1;
        }
        if (!device) {
            fprintf(stderr, "Error: --solver=gcr runs the device solver only (no --host)\n");
            return 1;
        }
        gcr = (int)k;
        if (precond == nullptr) precond = "none";
    } else if (strcmp(solver, "cg") != 0 && strcmp(solver, "bicgstab") != 0) {
        fprintf(stderr, "Error: unknown solver '%s' (cg, bicgstab, gcr[:M])\n", solver);
        return 1;
    }
    const bool bicgstab = !strcmp(solver, "bicgstab");
    if (bicgstab) {
        if (precond == nullptr) precond = "none";
        if (strcmp(precond, "none") != 0 && strcmp(precond, "jacobi") != 0) {
            fprintf(stderr, "Error: --solver=bicgstab takes --precond=none or --precond=jacobi, not '%s' (the other kinds are built for symmetric definite matrices)\n", precond);
            return 1;
        }
        if (!device) {
            fprintf(stderr, "Error: --solver=bicgstab runs the device solver only (no --host)\n");
            return 1;
        }
    }
    int cheb_degree = -1;  // >= 0: --precond=chebyshev[:K]
    int mg_degree = -1;    // >= 0: --precond=multigrid[:NU]
    int amg_degree = -1;   // >= 0: --precond=amg[:NU]
    if (precond && !strncmp(precond, "chebyshev", 9) && (precond[9] == '\0' || precond[9] == ':')) {
        char* end = nullptr;
        const long k = precond[9] == ':' ? strtol(precond + 10, &end, 10) : 4;
        if (precond[9] == ':' && (end == precond + 10 || *end != '\0' || k < 0 || k > 32)) {
            fprintf(stderr, "Error: --precond=chebyshev:K takes a degree K of 0..32, not '%s'\n", precond + 10);
            return 1;
        }
        cheb_degree = (int)k;
    } else if (precond && !strncmp(precond, "multigrid", 9) && (precond[9] == '\0' || precond[9] == ':')) {
        char* end = nullptr;
        const long k = precond[9] == ':' ? strtol(precond + 10, &end, 10) : 1;
        if (precond[9] == ':' && (end == precond + 10 || *end != '\0' || k < 0 || k > 8)) {
            fprintf(stderr, "Error: --precond=multigrid:NU takes a smoother degree NU of 0..8, not '%s'\n", precond + 10);
            return 1;
        }
        mg_degree = (int)k;
    } else if (precond && !strncmp(precond, "amg", 3) && (precond[3] == '\0' || precond[3] == ':')) {
        char* end = nullptr;
        const long k = precond[3] == ':' ? strtol(precond + 4, &end, 10) : 1;
        if (precond[3] == ':' && (end == precond + 4 || *end != '\0' || k < 0 || k > 8)) {
            fprintf(stderr, "Error: --precond=amg:NU takes a smoother degree NU of 0..8, not '%s'\n", precond + 4);
            return 1;
        }
        amg_degree = (int)k;
    } else if (precond && strcmp(precond, "none") != 0 && strcmp(precond, "jacobi") != 0) {
        fprintf(stderr, "Error: unknown preconditioner '%s' (none, jacobi)\n", precond);
        return 1;
    }
    if (precond && !device) {
        fprintf(stderr, "Error: --precond runs the device solver only (no --host)\n");
        return 1;
    }
    const std::vector<std::string> modes = app::split_modes(modes_text);
    for (const std::string& m : modes) {
        SpmvOperator* op = get_operator(m.c_str());
        if (!op) {
            fprintf(stderr, "Error: Unknown mode '%s'\n", m.c_str());
            return 1;
        }
        if (device && !op->run_device) {
            fprintf(stderr, "Error: mode '%s' has no device-native interface (use --host)\n", m.c_str());
            return 1;
        }
        if (amg_degree >= 0 && m != "cusparse-csr") {
            fprintf(stderr, "Error: --precond=amg runs on --mode=cusparse-csr only, not on '%s' (the stencil operators take --precond=multigrid)\n", m.c_str());
            return 1;
        }
    }
    MatrixData mat;
    if (stencil3d > 674) {
        fprintf(stderr, "Failed to build the %d^3 stencil (1 <= N <= 674)\n", stencil3d);
        return 1;
    }
    if (stencil3d > 0  ? !app::make_stencil3d(stencil3d, &mat)
        : stencil > 0 ? !app::make_stencil(stencil, &mat)
                      : load_matrix_market(matrix, &mat) != 0) {
        fprintf(stderr, "Error loading matrix\n");
        return 1;
    }
    printf("Matrix loaded: %d x %d, %d nonzeros\n", mat.rows, mat.cols, mat.nnz);
    std::vector<double> b((size_t)mat.rows, 1.0), x((size_t)mat.rows, 0.0);
    bool first_csv = true;
    for (const std::string& m : modes) {
        SpmvOperator* op = get_operator(m.c_str());
        printf("\n========================================\nCG Solver - Mode: %s\n========================================\n", m.c_str());
        printf("Interface: %s\nTolerance: %.1e, Max iterations: %d\n", device ? "Device-native (GPU)" : "Host", tol, maxiter);
        if (op->init(&mat) != 0) {
            fprintf(stderr, "Failed to initialize operator\n");
            continue;
        }
        CGConfig quiet = {maxiter, tol, 0, 0}, cfg = {maxiter, tol, 0, timers};
        CGStats st;
        if (precond) {
            int bad_row = -1;
            const bool is3d = op->name != nullptr && !strcmp(op->name, "stencil7-csr");
            SpmvAmdPrecond* pm = amg_degree >= 0        ? spmv_amd_precond_create_amg(op, amg_degree, 0, 0.08, &bad_row)
                                 : mg_degree >= 0 && is3d ? spmv_amd_precond_create_multigrid3d(op, mg_degree, 0, &bad_row)
                                 : mg_degree >= 0     ? spmv_amd_precond_create_multigrid(op, mg_degree, 0, &bad_row)
                                 : cheb_degree >= 0 ? spmv_amd_precond_create_chebyshev(op, cheb_degree, 0.0, 0.0, &bad_row)
                                                    : spmv_amd_precond_create(op, precond, &bad_row);
            if (pm == nullptr) {
                fprintf(stderr, "Failed to create the '%s' preconditioner (row %d)\n", precond, bad_row);
                op->free();
                continue;
            }
            const std::string kind = amg_degree >= 0    ? "amg" + std::to_string(amg_degree)
                                     : mg_degree >= 0   ? "multigrid" + std::to_string(mg_degree)
                                     : cheb_degree >= 0 ? "chebyshev" + std::to_string(cheb_degree)
                                                        : std::string(precond);
            const std::string name = gcr > 0 ? "gcr" + std::to_string(gcr) : std::string("bicgstab");
            const std::string tag = !bicgstab && gcr == 0 ? m + "+" + kind : kind == "none" ? m + "+" + name : m + "+" + kind + "+" + name;
            const PrecondSolve solve = bicgstab ? spmv_amd_bicgstab_solve_device : spmv_amd_pcg_solve_device;
            if (bicgstab) printf("Solver: BiCGSTAB\n");
            if (gcr > 0) printf("Solver: GCR(%d)\n", gcr);
            printf("Preconditioner: %s\nWarmup (3 runs)...\n", kind.c_str());
            BenchmarkStats bs;
            memset(&bs, 0, sizeof bs);
            bool ok = pcg_runs(op, &mat, pm, b.data(), x, quiet, 3, &bs, &st, solve, gcr) == 0;
            memset(&bs, 0, sizeof bs);
            if (ok) printf("Running benchmark (10 runs)...\n");
            ok = ok && pcg_runs(op, &mat, pm, b.data(), x, cfg, 10, &bs, &st, solve, gcr) == 0;
            spmv_amd_precond_destroy(pm);
            if (!ok) {
                fprintf(stderr, "benchmark failed\n");
                op->free();
                continue;
            }
            printf("Completed: %d valid runs, %d outliers removed\n", bs.valid_runs, bs.outliers_removed);
            printf("\n--- Results for %s ---\nConverged: %s in %d iterations\nTime (median): %.3f ms\n", tag.c_str(),
                   st.converged ? "YES" : "NO", st.iterations, bs.median_ms);
            printf("Stats: min=%.3f ms, max=%.3f ms, std=%.3f ms\n", bs.min_ms, bs.max_ms, bs.std_dev_ms);
            printf("\n=== Output Checksum ===\nSum(x):    %.16e\nNorm2(x):  %.16e\n", st.solution_sum, st.solution_norm);
            if (json) export_cg_json(app::per_mode_path(json, tag.c_str(), ".json").c_str(), tag.c_str(), &mat, &bs, &st);
            if (csv) {
                export_cg_csv(csv, tag.c_str(), &mat, &bs, &st, first_csv);
                first_csv = false;
            }
            op->free();
            continue;
        }
        printf("Warmup (3 runs)...\n");
        for (int w = 0; w < 3; ++w) {
            std::fill(x.begin(), x.end(), 0.0);
            if (device) cg_solve_device(op, &mat, b.data(), x.data(), quiet, &st);
            else cg_solve(op, &mat, b.data(), x.data(), quiet, &st);
        }
        std::fill(x.begin(), x.end(), 0.0);
        BenchmarkStats bs;
        memset(&bs, 0, sizeof bs);
        if (device) {
            printf("Running benchmark (10 runs)...\n");
            if (cg_benchmark_with_stats_device(op, &mat, b.data(), x.data(), cfg, 10, &bs, &st) != 0) {
                fprintf(stderr, "benchmark failed\n");
                op->free();
                continue;
            }
        } else {
            cg_solve(op, &mat, b.data(), x.data(), cfg, &st);
            bs.median_ms = st.time_total_ms;
            bs.valid_runs = 1;
        }
        printf("Completed: %d valid runs, %d outliers removed\n", bs.valid_runs, bs.outliers_removed);
        printf("\n--- Results for %s ---\nConverged: %s in %d iterations\nTime (median): %.3f ms\n", m.c_str(),
               st.converged ? "YES" : "NO", st.iterations, bs.median_ms);
        printf("Stats: min=%.3f ms, max=%.3f ms, std=%.3f ms\n", bs.min_ms, bs.max_ms, bs.std_dev_ms);
        printf("\n=== Output Checksum ===\nSum(x):    %.16e\nNorm2(x):  %.16e\n", st.solution_sum, st.solution_norm);
        if (json) export_cg_json(app::per_mode_path(json, m.c_str(), ".json").c_str(), m.c_str(), &mat, &bs, &st);
        if (csv) {
            export_cg_csv(csv, m.c_str(), &mat, &bs, &st, first_csv);
            first_csv = false;
        }
        op->free();
    }
    free(mat.entries);
    return 0;
}
