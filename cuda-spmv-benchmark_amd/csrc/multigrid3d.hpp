// multigrid3d.hpp -- the launches of the 3-D multigrid cycle (multigrid3d.hip): multigrid.hip's cycle and the LAB
// build's spmv_amd_mg_stage make them. A 3-D level is a complete 7-point CSR of an n x n x n grid ([D,N,W,C,E,S,U],
// stencil_geometry.hpp); n is passed beside the view, whose grid_size means "2-D 5-point". Default stream, no synchronisation.
#pragma once

#include "kernels.hpp"

namespace spmv_amd {

// the view of a complete 7-point CSR on an n^3 grid in the caller's arrays (2 <= n <= 674)
SlabCsr stencil7_view(int n, const int* row_ptr, const int* col_idx, const double* values);
// A_c = P^T A P on the ceil(n / 2)^3 grid, 2 x 2 x 2 aggregates, every entry a sequential sum in the order api.h states
void launch_coarsen3d(const SlabCsr& fine, int n, int* row_ptr, int* col_idx, double* values);
// r_c = P^T (r - A z) in one launch; A z and r - A z are never stored. z and r: 16-byte aligned.
void launch_residual_restrict3d(const SlabCsr& m, int n, const double* z, const double* r, double* rc);
// z = fma(2.0, e_c[agg(i)], z), z (16-byte aligned) in place
void launch_prolong_correct3d(int n, const double* ec, double* z);

// ---- the same two launches on block vectors of k = 1..8 row-interleaved columns (multigrid3d_multi.hip): the
// batched cycle of multigrid_multi.hip and the LAB build's spmv_amd_mg_multi_stage3d make them. cols: the device column records (null:
// every column is running); nothing is read or written once every column is done. Block vectors: 8-byte aligned, 16-byte accesses
// wherever an address allows. ----
struct PcgMultiColumn;
void launch_residual_restrict3d_multi(int k, const SlabCsr& m, int n, const PcgMultiColumn* cols, const double* z, const double* r, double* rc);
void launch_prolong_correct3d_multi(int k, int n, const PcgMultiColumn* cols, const double* ec, double* z);

}  // namespace spmv_amd
