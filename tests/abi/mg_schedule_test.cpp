// csrc/mg_schedule.hpp on a CPU: the header and standard headers only. For every case on the command line -- `levels degree` pairs; the
// coarsest level's degree is 8 -- it walks one V-cycle with an Ops that prints one line per call: "<level> <operation> <last>".
// tests/test_multigrid_host.py compares the lines with its own statement of the cycle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mg_schedule.hpp"

namespace {

struct Level {
    int degree;
    std::vector<double> coef;  // c0, h_1, g_1, ...: values that name their own place, so a swapped (g, h) shows
};

struct Printer {
    const Level* levels;
    int failures = 0;
    void term0(int l) { std::printf("%d term0 0\n", l); }
    void step(int l, double g, double h, bool last) {
        // which step of the level this (g, h) is: 0 for (c0, 0.0), k for (g_k, h_k)
        const std::vector<double>& c = levels[l].coef;
        int k = -1;
        if (g == c[0] && h == 0.0) k = 0;
        for (int s = 1; s <= levels[l].degree; ++s)
            if (g == c[2 * s] && h == c[2 * s - 1]) k = s;
        if (k < 0) ++failures;
        std::printf("%d step%d %d\n", l, k, last ? 1 : 0);
    }
    void restrict_residual(int l) { std::printf("%d restrict 0\n", l); }
    void prolong(int l) { std::printf("%d prolong 0\n", l); }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 == 0) return std::fprintf(stderr, "usage: mg_schedule_test levels degree [levels degree ...]\n"), 2;
    int failures = 0;
    for (int at = 1; at + 1 < argc; at += 2) {
        const int count = std::atoi(argv[at]), nu = std::atoi(argv[at + 1]);
        std::vector<Level> levels((size_t)count);
        for (int l = 0; l < count; ++l) {
            Level& L = levels[(size_t)l];
            L.degree = l + 1 == count ? 8 : nu;
            L.coef.resize(1 + 2 * (size_t)L.degree);
            for (size_t i = 0; i < L.coef.size(); ++i) L.coef[i] = 100.0 * (l + 1) + (double)i + 0.5;
        }
        std::printf("case %d %d\n", count, nu);
        Printer ops{levels.data()};
        spmv_amd::mg_vcycle(ops, levels.data(), count);
        failures += ops.failures;
    }
    std::printf(failures == 0 ? "mg_schedule: ok\n" : "mg_schedule: a step's (g, h) is not one of its level's\n");
    return failures == 0 ? 0 : 1;
}
