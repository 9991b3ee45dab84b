// multigrid3d.hip -- the device side of kind "multigrid" on the 3-D operator "stencil7-csr" (include/spmv_amd/api.h
// states the algebra down to the order of every sum): the three launches a 3-D level adds to multigrid.hip's cycle. The hierarchy, the
// cycle and the creator are multigrid.hip's; smoothing on a level is launch_stencil7_spmv + precond.hip's streaming step.
//
// Levels: n_{l+1} = ceil(n_l / 2); aggregate (K, I, J) = the fine points (2K + c, 2I + a, 2J + b), c, a, b in {0, 1}, that exist;
// A_c = P^T A P with P piecewise constant is again a complete 7-point CSR [D,N,W,C,E,S,U].
//   coarsen3d_kernel            one thread per coarse row; set-up work
//   residual_restrict3d_kernel  r_c = P^T (r - A z) in ONE launch: A z and r - A z never stored; 56 + 8 + 8 + 1 = 73 B per fine row
//   prolong_correct3d_kernel    z = fma(2.0, e_c[agg(i)], z), streaming
// Arithmetic: (A z)_i is stencil7-csr's row -- sum = fma(v[k], z[col[k]], sum) from +0.0 in ascending k, every row --, t = fma(-1.0,
// (A z)_i, r_i), r_c = (((((((t000 + t001) + t010) + t011) + t100) + t101) + t110) + t111) over the members that exist.
// -ffp-contract=off: the only fused multiply-adds are the explicit ones.
#include "multigrid.hpp"
#include "multigrid_device.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {
namespace {

constexpr hipStream_t kStream = nullptr;  // default stream, shared with the operators and pcg.hip
constexpr int kWave = 64;

// ---- coarsening ----
// Every coarse entry is a sequential sum from 0.0 with plain additions: the members in the order (c, a, b) = (0,0,0), (0,0,1), (0,1,0),
// ..., (1,1,1), each member's entries in CSR order, an entry added to the coarse entry of the aggregate its column lies in. A 7-point
// column differs from its row on ONE axis, so the aggregate it lies in is the row's own or a face neighbour.
__global__ __launch_bounds__(256) void coarsen3d_kernel(SlabCsr fine, int n, int nc, int* __restrict__ row_ptr, int* __restrict__ col_idx,
                                                        double* __restrict__ values) {
    const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int ncc = nc * nc;
    if (row >= ncc * nc) return;
    const int K = row / ncc, rest = row - K * ncc;
    const int I = rest / nc, J = rest - I * nc;
    const int nn = n * n;
    double vd = 0.0, vn = 0.0, vw = 0.0, vc = 0.0, ve = 0.0, vs = 0.0, vu = 0.0;
    for (int c = 0; c < 2; ++c) {
        for (int a = 0; a < 2; ++a) {
            for (int b = 0; b < 2; ++b) {
                const int k = 2 * K + c, i = 2 * I + a, j = 2 * J + b;
                if (k >= n || i >= n || j >= n) continue;
                const int fr = (k * n + i) * n + j;
                for (int e = fine.row_ptr[fr]; e < fine.row_ptr[fr + 1]; ++e) {
                    const int col = fine.col_idx[e];
                    const int ck = col / nn, crest = col - ck * nn;
                    const int ci = crest / n, cj = crest - ci * n;
                    const int CK = ck >> 1, CI = ci >> 1, CJ = cj >> 1;
                    const double v = fine.values[e];
                    if (CK < K) vd = vd + v;
                    else if (CK > K) vu = vu + v;
                    else if (CI < I) vn = vn + v;
                    else if (CI > I) vs = vs + v;
                    else if (CJ < J) vw = vw + v;
                    else if (CJ > J) ve = ve + v;
                    else vc = vc + v;
                }
            }
        }
    }
    int at = (int)stencil7_row_start(K, I, J, nc);
    row_ptr[row] = at;
    if (K > 0) col_idx[at] = row - ncc, values[at] = vd, ++at;
    if (I > 0) col_idx[at] = row - nc, values[at] = vn, ++at;
    if (J > 0) col_idx[at] = row - 1, values[at] = vw, ++at;
    col_idx[at] = row, values[at] = vc, ++at;
    if (J < nc - 1) col_idx[at] = row + 1, values[at] = ve, ++at;
    if (I < nc - 1) col_idx[at] = row + nc, values[at] = vs, ++at;
    if (K < nc - 1) col_idx[at] = row + ncc, values[at] = vu, ++at;
    if (row == ncc * nc - 1) row_ptr[ncc * nc] = at;
}

// ---- residual + restriction in one launch ----
// One one-wave workgroup takes (coarse plane K, coarse grid row I, 128 fine columns): 64 coarse values, lane l owns aggregate column l
// of the tile (fine columns ja = j0 + 2 l and jb = ja + 1) and walks the four fine grid rows (k, i) = (2K + c, 2I + a) in sum order.
// A block whose four grid rows are all inside the cube (1 <= 2K, 2K + 1 <= n - 2, the same for I) takes the fast path:
//   * z on the twelve grid rows the block touches -- its own four, and the N / S / D / U neighbours outside it, two each -- and r on
//     its own four: a 16-byte pair per lane and row where the pair is 16-byte aligned (an odd n leaves half the grid rows 8-byte
//     aligned only: two 8-byte loads there), each loaded ONCE and kept in registers; r nontemporal, z plain (the neighbouring blocks
//     read the same lines); every load is issued before the first use;
//   * per grid row its tile of coefficients -- 896 consecutive CSR values on a full tile, 56 B/row -- by fourteen coalesced
//     nontemporal 8-byte loads per lane into ONE wave-private LDS strip (stencil7_rowlds_kernel's layout: the run starts one entry
//     before the tile's first row, so column j0 + c sits at strip position 7 c: [D,N,W,C,E,S,U]; column 0 [D,N,C,E,S,U] at 1..6,
//     column n-1 [D,N,W,C,S,U] at 0..5). The next grid row's loads are in flight while this one's sums run. A short last tile loads
//     only the 7 * (live columns) entries that feed a row: the grid row's base is >= 1 and a following grid row exists, so no
//     address leaves the array and nothing is clamped;
//   * W of ja and E of jb from the adjacent lanes (a cross-lane move); only lane 0 and lane 63 load an outer column;
//   * one plain 8-byte store per lane: the next level reads it at once.
// A lane reads its two rows' slots at a lane stride of 14 doubles: lanes l and l + 16 of a 32-lane half share a bank (2-way, as the
// 2-D kernel's stride of 10; the strip's traffic is a fifth of what the coefficient loads take from HBM -- DESIGN.md section 17).
// LDS: 7 168 B per wave. Every other block -- a grid row on a face of the cube in it, the lone last plane or grid row of an odd n --
// goes one thread per aggregate through row_ptr (member_residual). Tiles are dealt to the XCDs by xcd_run_tile; the launcher pads.

// strip_row7, load_strip, load_pair and member_residual: multigrid_device.hpp
__global__ __launch_bounds__(kWave) void residual_restrict3d_kernel(SlabCsr m, int n, const double* __restrict__ z, const double* __restrict__ r,
                                                                    double* __restrict__ rc, int nc, int col_tiles, int total_tiles, int run) {
    __shared__ double strip[7 * kStripCols];
    const int tile = xcd_run_tile<int>((int)blockIdx.x, run);
    if (tile >= total_tiles) return;
    const int g = tile / col_tiles;  // the coarse grid row K nc + I
    const int j0 = (tile - g * col_tiles) * kStripCols;
    const int K = g / nc, I = g - K * nc;
    const int lane = (int)threadIdx.x;
    const int ja = j0 + 2 * lane, jb = ja + 1;
    const int k0 = 2 * K, i0 = 2 * I;
    const bool has_a = ja < n, has_b = jb < n;
    const long long nn = (long long)n * n;
    const long long out = (long long)g * nc + (ja >> 1);
    if (k0 >= 1 && k0 + 1 <= n - 2 && i0 >= 1 && i0 + 1 <= n - 2) {
        const int live = n - j0 < kStripCols ? n - j0 : kStripCols;
        const int entries = 7 * live;
        double c[14];
        load_strip(m.values + (stencil7_row_start(k0, i0, 0, n) + 7LL * j0 - 1 + lane), lane, entries, c);
        // z: own[c][a] the block's four grid rows; zn / zs: grid rows i0 - 1 / i0 + 2 of plane k0 + c; zd / zu: planes k0 - 1 / k0 + 2 of grid row i0 + a
        d2 own[2][2], zn[2], zs[2], zd[2], zu[2], rv[2][2];
        double west[2][2], east[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            zn[q] = zs[q] = zd[q] = zu[q] = d2{0.0, 0.0};
#pragma unroll
            for (int a = 0; a < 2; ++a) own[q][a] = rv[q][a] = d2{0.0, 0.0}, west[q][a] = east[q][a] = 0.0;
        }
        if (has_a) {
            const long long at = (long long)k0 * nn + (long long)i0 * n + ja;  // (k0, i0, ja)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const long long p = at + q * nn + a * n;
                    own[q][a] = load_pair<false>(z, p, has_b);
                    rv[q][a] = load_pair<true>(r, p, has_b);
                    if (lane == 0 && ja > 0) west[q][a] = z[p - 1];
                    if (lane == 63 && jb + 1 < n) east[q][a] = z[p + 2];
                }
                zn[q] = load_pair<false>(z, at + q * nn - n, has_b);
                zs[q] = load_pair<false>(z, at + q * nn + 2 * n, has_b);
                zd[q] = load_pair<false>(z, at - nn + q * n, has_b);
                zu[q] = load_pair<false>(z, at + 2 * nn + q * n, has_b);
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int s = 0; s < 14; ++s) strip[64 * s + lane] = c[s];
                wave_lds_sync();
                if (q * 2 + a < 3) {  // the next grid row's coefficients fly while this one's sums run
                    const int qn = a == 1 ? q + 1 : q, an = a == 1 ? 0 : 1;
                    load_strip(m.values + (stencil7_row_start(k0 + qn, i0 + an, 0, n) + 7LL * j0 - 1 + lane), lane, entries, c);
                }
                const d2 xc = own[q][a];
                const d2 xn = a == 0 ? zn[q] : own[q][0], xs = a == 1 ? zs[q] : own[q][1];
                const d2 xd = q == 0 ? zd[a] : own[0][a], xu = q == 1 ? zu[a] : own[1][a];
                const double from_west = __shfl_up(xc.y, 1), from_east = __shfl_down(xc.x, 1);
                const double xw_a = lane > 0 ? from_west : west[q][a];
                const double xe_b = lane < 63 ? from_east : east[q][a];
                if (has_a) {
                    const double* __restrict__ v = strip + 7 * (2 * lane);
                    const double ta = fma(-1.0, strip_row7(v, ja, n, xd.x, xn.x, xw_a, xc.x, xc.y, xs.x, xu.x), rv[q][a].x);
                    acc = (q == 0 && a == 0) ? ta : acc + ta;
                    if (has_b) {
                        const double tb = fma(-1.0, strip_row7(v + 7, jb, n, xd.y, xn.y, xc.x, xc.y, xe_b, xs.y, xu.y), rv[q][a].y);
                        acc = acc + tb;
                    }
                }
                wave_lds_sync();  // the next grid row's strip stores stay behind these reads
            }
        }
        if (has_a) rc[out] = acc;
    } else if (has_a) {
        // a grid row on a face of the cube in the block, a lone last plane or grid row: one thread per aggregate, the members that exist
        double acc = 0.0;
        for (int q = 0; q < 2; ++q) {
            for (int a = 0; a < 2; ++a) {
                if (k0 + q >= n || i0 + a >= n) continue;
                const long long row = (long long)(k0 + q) * nn + (long long)(i0 + a) * n + ja;
                const double ta = member_residual(m, z, r, row);
                acc = (q == 0 && a == 0) ? ta : acc + ta;
                if (has_b) acc = acc + member_residual(m, z, r, row + 1);
            }
        }
        rc[out] = acc;
    }
}

// ---- prolongation + correction: z = fma(2.0, e_c[agg(i)], z), z in place; one-wave workgroups, a 16-byte pair per lane ----
// coarse_at3d (multigrid_device.hpp): e_c at the aggregate of a flat fine row
__global__ __launch_bounds__(kWave) void prolong_correct3d_kernel(unsigned rows, unsigned n, unsigned nc, const double* __restrict__ ec,
                                                                  double* __restrict__ z) {
    const unsigned i = blockIdx.x * kWave + threadIdx.x;
    if (i < (rows >> 1)) {
        d2 zv = reinterpret_cast<const d2*>(z)[i];
        zv.x = fma(2.0, coarse_at3d(ec, 2 * i, n, nc), zv.x);
        zv.y = fma(2.0, coarse_at3d(ec, 2 * i + 1, n, nc), zv.y);
        reinterpret_cast<d2*>(z)[i] = zv;  // plain: the post-smoother's SpMV reads it
    }
    if ((rows & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[rows - 1] = fma(2.0, coarse_at3d(ec, rows - 1, n, nc), z[rows - 1]);
}

}  // namespace

// ---- the launches ----
SlabCsr stencil7_view(int n, const int* row_ptr, const int* col_idx, const double* values) {
    SlabCsr v;
    v.row_ptr = row_ptr, v.col_idx = col_idx, v.values = values;
    v.n_local = v.n_global = n * n * n;
    v.nnz_local = stencil7_nnz(n);
    v.max_row_nnz = n >= 3 ? 7 : 4;
    return v;  // grid_size stays unset: it means "2-D 5-point" to the kernels that read it
}

void launch_coarsen3d(const SlabCsr& fine, int n, int* row_ptr, int* col_idx, double* values) {
    const int nc = coarse_grid_of(n);
    const int rows = nc * nc * nc;
    hipLaunchKernelGGL(coarsen3d_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, kStream, fine, n, nc, row_ptr, col_idx, values);
}

void launch_residual_restrict3d(const SlabCsr& m, int n, const double* z, const double* r, double* rc) {
    const RestrictTiles t = restrict_tiles7(n);
    hipLaunchKernelGGL(residual_restrict3d_kernel, dim3(t.grid()), dim3(kWave), 0, kStream, m, n, z, r, rc, t.nc, t.col_tiles, t.tiles, t.run);
}

void launch_prolong_correct3d(int n, const double* ec, double* z) {
    const size_t rows = (size_t)n * n * n;  // <= 674^3 < 2^31
    hipLaunchKernelGGL(prolong_correct3d_kernel, dim3(stream_grid(rows)), dim3(kWave), 0, kStream, (unsigned)rows, (unsigned)n,
                       (unsigned)coarse_grid_of(n), ec, z);
}

}  // namespace spmv_amd
