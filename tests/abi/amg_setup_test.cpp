// csrc/amg_setup.hpp on a CPU: the header and standard headers only. Reads one matrix per file named on the command line -- the line
// "rows nnz theta max_levels" (theta a hex double), then rows + 1 row pointers, nnz columns and nnz values as hex doubles -- builds the
// whole hierarchy and prints it: per level "level <l> <rows> <nnz> <aggregates> <largest>", then the lines "rp ...", "ci ...",
// "va ..." (hex doubles) and, for a level that is not the coarsest, "agg ...", "ptr ..." and "mem ...". tests/test_amg_host.py
// compares the lines with tests/amg_restatement.py bit for bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "amg_setup.hpp"

namespace {

void print_ints(const char* tag, const std::vector<int>& v) {
    std::printf("%s", tag);
    for (const int x : v) std::printf(" %d", x);
    std::printf("\n");
}

bool read_matrix(const char* path, spmv_amd::amg::HostCsr* A, double* theta, int* max_levels) {
    std::FILE* f = std::fopen(path, "r");
    if (f == nullptr) return false;
    int rows = 0;
    long long nnz = 0;
    char word[64];
    bool ok = std::fscanf(f, "%d %lld %63s %d", &rows, &nnz, word, max_levels) == 4 && rows >= 1 && nnz >= 0;
    if (ok) {
        *theta = std::strtod(word, nullptr);
        A->row_ptr.assign((size_t)rows + 1, 0);
        A->col_idx.assign((size_t)nnz, 0);
        A->values.assign((size_t)nnz, 0.0);
        for (int& p : A->row_ptr) ok = ok && std::fscanf(f, "%d", &p) == 1;
        for (int& c : A->col_idx) ok = ok && std::fscanf(f, "%d", &c) == 1 && c >= 0 && c < rows;
        for (double& v : A->values) {
            ok = ok && std::fscanf(f, "%63s", word) == 1;
            if (ok) v = std::strtod(word, nullptr);
        }
        ok = ok && A->row_ptr.front() == 0 && A->row_ptr.back() == nnz;
        for (int i = 0; ok && i < rows; ++i) ok = A->row_ptr[(size_t)i] <= A->row_ptr[(size_t)i + 1];
    }
    std::fclose(f);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return std::fprintf(stderr, "usage: amg_setup_test matrix.txt [matrix.txt ...]\n"), 2;
    for (int at = 1; at < argc; ++at) {
        spmv_amd::amg::HostCsr A;
        double theta = 0.0;
        int max_levels = 0;
        if (!read_matrix(argv[at], &A, &theta, &max_levels)) return std::fprintf(stderr, "amg_setup_test: cannot read %s\n", argv[at]), 2;
        std::printf("matrix %s\n", argv[at]);
        const std::vector<spmv_amd::amg::HostLevel> levels = spmv_amd::amg::hierarchy(std::move(A), theta, max_levels);
        for (size_t l = 0; l < levels.size(); ++l) {
            const spmv_amd::amg::HostLevel& L = levels[l];
            std::printf("level %zu %d %lld %d %d\n", l, L.A.rows(), L.A.nnz(), L.g.count, L.g.max_aggregate);
            print_ints("rp", L.A.row_ptr);
            print_ints("ci", L.A.col_idx);
            std::printf("va");
            for (const double v : L.A.values) std::printf(" %a", v);
            std::printf("\n");
            if (L.g.count > 0) {
                print_ints("agg", L.g.agg);
                print_ints("ptr", L.g.agg_ptr);
                print_ints("mem", L.g.members);
            }
        }
    }
    std::printf("amg_setup: ok\n");
    return 0;
}
