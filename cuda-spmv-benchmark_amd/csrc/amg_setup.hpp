// amg_setup.hpp -- the host set-up of the aggregation AMG hierarchy (include/spmv_amd/api.h states the rules
// under spmv_amd_precond_create_amg): the strong couplings, the three aggregation passes, the member lists and the Galerkin product
// A_c = P^T A P on host CSR arrays. Standard headers only: no HIP, nothing here launches, so tests/abi/amg_setup_test.cpp walks it on a
// CPU under sanitizers. Every operation is fp64 with one rounding; no expression here has the form a * b + c, so a compiler that
// contracts has nothing to contract. The set-up is sequential by definition: aggregates are numbered in order of creation.
#ifndef SPMV_AMD_AMG_SETUP_HPP
#define SPMV_AMD_AMG_SETUP_HPP

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace spmv_amd {
namespace amg {

constexpr int kCoarsestRows = 64;  // a level of at most this many rows is the coarsest
constexpr int kMaxLevels = 32;     // max_levels 0 (automatic) means this

struct HostCsr {
    std::vector<int> row_ptr{0};
    std::vector<int> col_idx;
    std::vector<double> values;
    int rows() const { return (int)row_ptr.size() - 1; }
    long long nnz() const { return (long long)col_idx.size(); }
    int max_row_nnz() const {
        int longest = 0;
        for (int i = 0; i < rows(); ++i) longest = std::max(longest, row_ptr[(size_t)i + 1] - row_ptr[(size_t)i]);
        return longest;
    }
};

// The diagonal pass: d_i = the sum of row i's entries in column i, CSR order, from 0.0.
inline std::vector<double> diagonal(const HostCsr& A) {
    std::vector<double> d((size_t)A.rows(), 0.0);
    for (int i = 0; i < A.rows(); ++i)
        for (int k = A.row_ptr[(size_t)i]; k < A.row_ptr[(size_t)i + 1]; ++k)
            if (A.col_idx[(size_t)k] == i) d[(size_t)i] = d[(size_t)i] + A.values[(size_t)k];
    return d;
}

// Entry k of row i (column j != i, value v) is strong iff v * v > t2 * fabs(d_i * d_j), t2 = theta * theta.
inline bool strong(const HostCsr& A, const std::vector<double>& d, double t2, int i, int k) {
    const int j = A.col_idx[(size_t)k];
    if (j == i) return false;
    const double v = A.values[(size_t)k];
    const double dd = d[(size_t)i] * d[(size_t)j];
    return v * v > t2 * std::fabs(dd);
}

struct Aggregates {
    int count = 0;
    std::vector<int> agg;      // rows: the aggregate of each row
    std::vector<int> agg_ptr;  // count + 1
    std::vector<int> members;  // rows: each aggregate's rows in ascending order
    int max_aggregate = 0;
};

// The three passes, in ascending row order; then the member lists.
inline Aggregates aggregate(const HostCsr& A, const std::vector<double>& d, double theta) {
    const int n = A.rows();
    const double t2 = theta * theta;
    Aggregates g;
    g.agg.assign((size_t)n, -1);
    // pass 1: a row none of whose strong neighbours is aggregated founds an aggregate with all of them
    for (int i = 0; i < n; ++i) {
        if (g.agg[(size_t)i] >= 0) continue;
        bool is_free = true;
        for (int k = A.row_ptr[(size_t)i]; is_free && k < A.row_ptr[(size_t)i + 1]; ++k)
            if (strong(A, d, t2, i, k) && g.agg[(size_t)A.col_idx[(size_t)k]] >= 0) is_free = false;
        if (!is_free) continue;
        g.agg[(size_t)i] = g.count;
        for (int k = A.row_ptr[(size_t)i]; k < A.row_ptr[(size_t)i + 1]; ++k)
            if (strong(A, d, t2, i, k)) g.agg[(size_t)A.col_idx[(size_t)k]] = g.count;
        ++g.count;
    }
    // pass 2, on a copy of pass 1's map: a row joins the aggregate of its first strong neighbour pass 1 placed
    {
        const std::vector<int> first = g.agg;
        for (int i = 0; i < n; ++i) {
            if (first[(size_t)i] >= 0) continue;
            for (int k = A.row_ptr[(size_t)i]; k < A.row_ptr[(size_t)i + 1]; ++k) {
                if (!strong(A, d, t2, i, k) || first[(size_t)A.col_idx[(size_t)k]] < 0) continue;
                g.agg[(size_t)i] = first[(size_t)A.col_idx[(size_t)k]];
                break;
            }
        }
    }
    // pass 3: what is left founds aggregates with its strong neighbours that are still left
    for (int i = 0; i < n; ++i) {
        if (g.agg[(size_t)i] >= 0) continue;
        g.agg[(size_t)i] = g.count;
        for (int k = A.row_ptr[(size_t)i]; k < A.row_ptr[(size_t)i + 1]; ++k)
            if (strong(A, d, t2, i, k) && g.agg[(size_t)A.col_idx[(size_t)k]] < 0) g.agg[(size_t)A.col_idx[(size_t)k]] = g.count;
        ++g.count;
    }
    // member lists: a counting sort by aggregate keeps the rows ascending
    g.agg_ptr.assign((size_t)g.count + 1, 0);
    for (int i = 0; i < n; ++i) ++g.agg_ptr[(size_t)g.agg[(size_t)i] + 1];
    for (int I = 0; I < g.count; ++I) {
        g.max_aggregate = std::max(g.max_aggregate, g.agg_ptr[(size_t)I + 1]);
        g.agg_ptr[(size_t)I + 1] += g.agg_ptr[(size_t)I];
    }
    g.members.assign((size_t)n, 0);
    std::vector<int> at(g.agg_ptr.begin(), g.agg_ptr.end() - 1);
    for (int i = 0; i < n; ++i) g.members[(size_t)at[(size_t)g.agg[(size_t)i]]++] = i;
    return g;
}

// Level `level` (of `rows` rows) is the coarsest before any aggregation: few rows, or the cap on levels.
inline bool coarsest_by_size(int rows, int level, int max_levels) {
    return rows <= kCoarsestRows || level + 1 == (max_levels > 0 ? max_levels : kMaxLevels);
}
// ... or after it: an aggregation that keeps more than nine tenths of the rows is discarded.
inline bool coarsens_too_little(int rows, int coarse_rows) { return 10LL * coarse_rows > 9LL * rows; }

// A_c = P^T A P, P piecewise constant over g. Row I holds one entry per distinct aggregate J = agg(col) its members' rows meet, sorted
// by ascending J, stored zeros kept; each value a plain sequential sum that starts from its first term: the members in ascending
// order, each member's entries in CSR order. Rows of any length: the open row lives in two vectors that grow, found through a
// marker per coarse column.
inline HostCsr galerkin(const HostCsr& A, const Aggregates& g) {
    HostCsr C;
    C.row_ptr.assign((size_t)g.count + 1, 0);
    std::vector<int> slot((size_t)g.count, -1);  // coarse column -> its place in the open row
    std::vector<int> cols;
    std::vector<double> vals;
    std::vector<std::pair<int, double>> sorted;
    for (int I = 0; I < g.count; ++I) {
        cols.clear(), vals.clear();
        for (int m = g.agg_ptr[(size_t)I]; m < g.agg_ptr[(size_t)I + 1]; ++m) {
            const int i = g.members[(size_t)m];
            for (int k = A.row_ptr[(size_t)i]; k < A.row_ptr[(size_t)i + 1]; ++k) {
                const int J = g.agg[(size_t)A.col_idx[(size_t)k]];
                const double v = A.values[(size_t)k];
                if (slot[(size_t)J] < 0) {
                    slot[(size_t)J] = (int)cols.size();
                    cols.push_back(J), vals.push_back(v);
                } else {
                    vals[(size_t)slot[(size_t)J]] = vals[(size_t)slot[(size_t)J]] + v;
                }
            }
        }
        sorted.clear();
        for (size_t q = 0; q < cols.size(); ++q) sorted.emplace_back(cols[q], vals[q]), slot[(size_t)cols[q]] = -1;
        std::sort(sorted.begin(), sorted.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
        for (const auto& e : sorted) C.col_idx.push_back(e.first), C.values.push_back(e.second);
        C.row_ptr[(size_t)I + 1] = (int)C.col_idx.size();
    }
    return C;
}

// One level of the hierarchy on the host: its matrix and, unless it is the coarsest, its aggregates.
struct HostLevel {
    HostCsr A;
    Aggregates g;  // count == 0: the coarsest level
};

// The whole hierarchy from level 0's matrix. Column indices must lie in [0, rows).
inline std::vector<HostLevel> hierarchy(HostCsr A0, double theta, int max_levels) {
    std::vector<HostLevel> levels;
    levels.emplace_back();
    levels.back().A = std::move(A0);
    for (int l = 0;; ++l) {
        const int rows = levels[(size_t)l].A.rows();  // by value: emplace_back below moves the levels
        if (coarsest_by_size(rows, l, max_levels)) break;
        Aggregates g = aggregate(levels[(size_t)l].A, diagonal(levels[(size_t)l].A), theta);
        if (coarsens_too_little(rows, g.count)) break;
        HostCsr C = galerkin(levels[(size_t)l].A, g);
        levels[(size_t)l].g = std::move(g);
        levels.emplace_back();
        levels.back().A = std::move(C);
    }
    return levels;
}

}  // namespace amg
}  // namespace spmv_amd
#endif
