// rowlds_tile_device.hpp -- the row-lds tile of the STENCIL5 SpMV: 128 columns of one grid row, evaluated by one wave, and the
// reference-order row (row_reference) it and the one-thread-per-row kernels fall back to. Shared by the one-row kernels (spmv_kernels.hip)
// and the block-tile kernels (stencil5_block_kernels.hip), whose tiles that are not uniform call it once per grid row: a row's bits do
// not depend on the launch it falls in.
#pragma once

#include <type_traits>

#include "kernels.hpp"
#include "reduce_device.hpp"
#include "stencil_geometry.hpp"
#include "stencil_row_device.hpp"
#include "stream_device.hpp"

namespace spmv_amd {

// x[col - row_offset] if that index is readable, else 0 (halo kernel semantics,
// reference src/spmv/spmv_stencil_partitioned_halo_kernel.cu:77-94).
__device__ __forceinline__ double x_at(const double* __restrict__ x, long long local_col,
                                       int lo, int hi) {
    return (local_col >= lo && local_col < hi) ? x[local_col] : 0.0;
}

// One row, evaluated the way the reference kernels do: computed offset and computed
// columns for interior rows of a verified stencil, the CSR loop otherwise.
template <bool kAnalyticInterior>
__device__ __forceinline__ double row_reference(const SlabCsr& m, const double* __restrict__ x,
                                                int local_row, int i, int j) {
    const int n = m.grid_size;
    if (kAnalyticInterior && stencil_is_interior(i, j, n)) {
        const long long o = stencil_row_start(i, j, n) - m.nnz_base;
        const double* __restrict__ v = m.values + o;
        const double* __restrict__ xl = x + local_row;
        return stencil5_interior(v[1], xl[-1], v[2], xl[0], v[3], xl[1], v[0], xl[-n], v[4], xl[n]);  // [N,W,C,E,S]
    }
    const int lo = -m.halo_before, hi = m.n_local + m.halo_after;
    const int k0 = m.row_ptr[local_row], k1 = m.row_ptr[local_row + 1];
    double sum = 0.0;
    for (int k = k0; k < k1; ++k)
        sum = fma(m.values[k], x_at(x, (long long)m.col_idx[k] - m.row_offset, lo, hi), sum);
    return sum;
}

// ---------------------------------------------------------------------------------
// STENCIL5, row-lds variant (default on slabs made of whole grid rows, n >= 512). Same index space
// as row-direct -- a workgroup is a run of columns of ONE grid row, so no thread divides -- but the
// coefficients take the streaming path the probes found fastest on MI355X
// (tools/stream_probe3.hip, profiles/r01_stream_probe3.txt):
//   * a workgroup is ONE wavefront that owns 128 consecutive columns, two rows per lane (columns
//     j0 + lane and j0 + 64 + lane): every x / y access stays an 8-byte-per-lane coalesced access;
//   * the tile's 640 coefficients are one contiguous run of `values` (five entries per interior
//     row): ten fully coalesced 8-byte NONTEMPORAL loads per lane -- the run is read once and never
//     again, so it should not displace x in L2 / Infinity Cache -- parked in a 5 KiB wave-private
//     LDS strip and read back as [N,W,C,E,S] per row (lane stride 40 B = 10 banks, an even stride
//     over 64 banks: conflict-free for 8-byte reads);
//   * y leaves with a nontemporal store;
//   * x: centre and N/S (the lines the neighbouring grid rows pull through L2 / Infinity Cache) by plain
//     loads: these are the re-used bytes. W/E come from a 1 KiB LDS copy of the tile's own centre values
//     (only the tile's two outer neighbours are loaded): four fewer vector-memory instructions per wave,
//     0.8 % at 20 000^2 and 2.6 % at 10 000^2, bit-identical results;
//   * tile -> XCD: workgroups are dealt round-robin to the eight XCDs, so tile = blockIdx would
//     scatter every 1 KiB of x / y over eight L2s. Instead each XCD takes `group` consecutive tiles
//     of every run of 8 * group (group = 4: 512 columns = 4 KiB of x and y, 20 KiB of values per
//     XCD and run). Measured at 20 000^2 with the real coefficient layout: group 1 3.89 ms,
//     group 2 4.04 ms, group 4 / 8 3.63 ms, group 16 3.73 ms -- a plateau, not a spike.
// Columns 0 and n-1 of an interior grid row (4-entry rows) are evaluated from the same strip in the
// CSR loop's order (ascending column, sum started at 0: reference :116-119); only the first and
// last grid row of the whole grid, whose rows have no N or S entry, walk row_ptr / col_idx.
// No barrier: the strip is private to the wave, and LDS operations of one wave retire in order.
// Arithmetic per interior row is exactly row-direct's (and the reference's) W,C,E,N,S fma chain.
// ---------------------------------------------------------------------------------
constexpr int kLdsTileCols = 128;

// kMode 0: y = alpha A x. kMode 1: also one partial of x . (A x) per wave (the CG loop's p.Ap).
// kMode 2 (first SpMV of a solve, x = the initial guess): y is NOT stored; instead r = b - A x (one fma, the
// reference's axpy_kernel(-1, Ap, b), mgpu :475), p = r, and one partial of r.r per wave -- the initial residual
// without writing A x0 out and reading it back (16 B/row less, once per solve).
// kMode 3 (one step of the Chebyshev preconditioner, x = z; kernels.hpp ChebStep): y is NOT stored; the row's sum stays in registers
// and runs t = fma(-1, sum, r), u = dinv t, d = fma(g, u, h d), z_out = z + d. r, dinv and d are read once (nontemporal, requested
// with the tile's x loads), d is written back in place, z_out -- another vector than x: neighbouring tiles still read x -- with a
// plain store, because the next step reads it as x. The last step of an application also leaves one partial of r . z_out per wave.
// 88 B per interior row (40 coefficients; z, r, dinv, d in; d, z_out out) against 56 + 56 for a SpMV followed by a streaming pass.
//
// One tile = local grid row li (global gi), columns [j0, j0 + 128), evaluated by one wave on its private LDS (`strip`:
// 640 doubles, `xrow`: 130). Returns false if the launch was enqueued past convergence (`skip`: the flag's value,
// REQUESTED by the caller before this call and tested here only after the tile's loads have been issued -- a wave does not
// sit on a scalar-load round trip before its first vector load; such a launch only reads). *dot: the tile's partial.
// kFreshHalo (boundary tiles evaluated behind a device-side arrival flag instead of a kernel boundary, see
// stencil5_rowlds_edges_reduce_kernel): the north / south values -- the halo rows another GPU's data was received into -- are
// read with SYSTEM-scope loads: the writer is another agent (a peer GPU's stores over xGMI, or the RCCL receive kernel acting
// for it), and no cache of this device may answer from a line it held before those rows arrived (2 x grid_size
// values per iteration, nothing on the clock).
// kSym (the symmetric coefficient form of a solver slab, kernels.hpp SymPlanes): interior grid rows take C and E from the [C, E]
// plane (one nontemporal 16-byte load per lane and row: read once per SpMV), S from the S plane and N = S[i - n] from the row
// one grid row up (plain loads: the S line is re-read as N one grid row later, like x's N / S neighbours), and W = E[i - 1]
// from the LDS copy of the tile's own E values (`strip`; lane 0 loads the one outside the tile). 24 B/row of coefficients
// instead of 40. The fma chains are the CSR form's, value for value (the planes were verified bit for bit at creation).
// tile_class (kSym only; rowlds_tile_class, the same value in every lane): 1 = every coefficient this tile multiplies equals the
// slab-wide quintuple in sp bit for bit (checked against the CSR at creation): the tile loads no coefficient, keeps no LDS copy of
// E and runs the same chains on the quintuple -- 0 B/row of coefficients. 0 = the plane path.
// kZeroX (kMode 2 only; stencil5_rowlds_zero_kernel): the caller knows that x holds +0.0 in every element. An interior grid row
// requests no x value: centre, W, E, N and S are 0.0 in registers, the LDS copy of the x row and its W / E exchange are gone, and
// everything behind the loads is the code of the other form -- the chains still multiply every coefficient by its zero, so -0.0
// and the NaN of an infinite coefficient come out bit for bit. The grid's first and last grid row read x as before.
template <int kMode, bool kFreshHalo = false, bool kSym = false, bool kZeroX = false>
__device__ __forceinline__ bool rowlds_tile(const SlabCsr& m, const double* __restrict__ x, double* __restrict__ y, double alpha,
                                            int li, int gi, int j0, int lane, int skip, double* __restrict__ strip,
                                            double* __restrict__ xrow, const ResidualOut& res, double* dot, const SymPlanes& sp = SymPlanes{},
                                            int tile_class = 0, const ChebStep& step = ChebStep{}) {
    constexpr bool kDot = kMode == 1;
    constexpr bool kInit = kMode == 2;
    constexpr bool kCheb = kMode == 3;
    const int n = m.grid_size;
    double dot_acc = 0.0;
    if (gi > 0 && gi < n - 1) {
        // slab-local position of the tile's first coefficient: row (gi, j) starts at base + 5 j - 1
        // for j >= 1; the run of the first tile starts one entry early so that row j sits at strip
        // position 5 j there too (row 0 itself holds [N,C,E,S] at positions 1..4)
        const long long e = stencil_gridrow_base(gi, n) + 5LL * j0 - 1 - m.nnz_base + lane;
        const double* __restrict__ vals = m.values;
        double c[10];
        d2 ce[2];                             // kSym: [C, E] of the lane's two rows
        double cs[2], cn[2], cw = 0.0;        // kSym: S, N = S[i - n]; lane 0: E[i - 1] of the tile's first row
        if constexpr (kSym) {
            // the plane loads are issued behind the x loads below: those do not depend on the tile's class, which is still on its way
        } else if (j0 == 0 || j0 + kLdsTileCols > n - 1) {
            // first / last tile of the grid row: part of the run lies outside the row (at the slab's
            // ends: outside the array): clamp the addresses, those strip slots feed no row
            const long long hi = m.nnz_local - 1;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                long long idx = e + 64 * k;
                idx = idx < 0 ? 0 : (idx > hi ? hi : idx);
                c[k] = __builtin_nontemporal_load(vals + idx);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 10; ++k) c[k] = __builtin_nontemporal_load(vals + e + 64 * k);
        }
        double xc[2], xw[2], xe[2], xn[2], xs[2], bv[2];
        double cr[2] = {0.0, 0.0}, cdv[2] = {0.0, 0.0}, cd[2] = {0.0, 0.0};  // kCheb: r, dinv and d of the lane's two rows
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + lane + 64 * h;
            xc[h] = xw[h] = xe[h] = xn[h] = xs[h] = bv[h] = 0.0;
            if (j < n) {
                const double* __restrict__ xl = x + ((long long)li * n + j);
                if constexpr (!kZeroX) {
                    xc[h] = xl[0];
                    if (kFreshHalo) {
                        xn[h] = published_by_any_agent(reinterpret_cast<const unsigned long long*>(xl - n));
                        xs[h] = published_by_any_agent(reinterpret_cast<const unsigned long long*>(xl + n));
                    } else {
                        xn[h] = xl[-n], xs[h] = xl[n];
                    }
                }
                if (kInit) bv[h] = __builtin_nontemporal_load(res.b + ((long long)li * n + j));
                if constexpr (kCheb) {  // streams read once per step, requested with the x loads (before the skip flag is tested)
                    cr[h] = __builtin_nontemporal_load(step.r + ((long long)li * n + j));
                    cdv[h] = __builtin_nontemporal_load(step.dinv + ((long long)li * n + j));
                    cd[h] = __builtin_nontemporal_load(step.d + ((long long)li * n + j));
                }
                // only the tile's two outer neighbours come from memory; the rest from the LDS copy below
                if constexpr (!kZeroX) {
                    if (h == 0 && lane == 0 && j > 0) xw[0] = xl[-1];
                    if (h == 1 && lane == 63 && j < n - 1) xe[1] = xl[1];
                }
            }
        }
        // Everything behind the tile's loads, for a tile that streams its coefficients (kUniform false: the CSR strip or the planes)
        // or one that takes the slab-wide quintuple (kUniform true). Two instances rather than one with selects: each keeps the
        // registers of its own path.
        const auto finish = [&](auto uniform_tile) {
            constexpr bool kUniform = decltype(uniform_tile)::value;
            if constexpr (kSym) {
                if constexpr (!kUniform) {
                    strip[1 + lane] = ce[0].y;
                    strip[65 + lane] = ce[1].y;
                    if (lane == 0) strip[0] = cw;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 10; ++k) strip[64 * k + lane] = c[k];
            }
            if constexpr (!kZeroX) {
                xrow[1 + lane] = xc[0];
                xrow[65 + lane] = xc[1];
            }
            wave_lds_sync();
            if constexpr (!kZeroX) tile_west_east(xrow, lane, j0, n, xw[0], xe[1], xw, xe);  // else: W and E are the zeros they were set to
            double cwv[2] = {0.0, 0.0};  // kSym: W = E[i - 1]
            if constexpr (kSym && !kUniform) {
                cwv[0] = strip[lane];
                cwv[1] = strip[64 + lane];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = j0 + lane + 64 * h;
                if (j < n) {
                    const double* __restrict__ v = strip + 5 * (lane + 64 * h);
                    double sum;
                    if constexpr (kSym) {
                        // a uniform tile: the quintuple, bit for bit what every row of the tile holds (checked against the CSR at creation)
                        const double vw = kUniform ? sp.w : cwv[h], vc = kUniform ? sp.c : ce[h].x, ve = kUniform ? sp.e : ce[h].y,
                                     vn = kUniform ? sp.n : cn[h], vs = kUniform ? sp.s5 : cs[h];
                        sum = stencil5_row(j, n, vw, xw[h], vc, xc[h], ve, xe[h], vn, xn[h], vs, xs[h]);
                    }
                    // The CSR strip form: its three chains (stencil_row_device.hpp's, on other strip slots per case) stay written out here;
                    // profiles/r14_stencil_helpers_isa_identity.txt, class C site 2, says why.
                    else if (j > 0 && j < n - 1) {       // [N,W,C,E,S], evaluated W,C,E,N,S
                        sum = v[1] * xw[h];
                        sum = fma(v[2], xc[h], sum);
                        sum = fma(v[3], xe[h], sum);
                        sum = fma(v[0], xn[h], sum);
                        sum = fma(v[4], xs[h], sum);
                    } else if (j == 0) {                 // [N,C,E,S] at strip positions 1..4, CSR-loop order
                        sum = fma(v[1], xn[h], 0.0);
                        sum = fma(v[2], xc[h], sum);
                        sum = fma(v[3], xe[h], sum);
                        sum = fma(v[4], xs[h], sum);
                    } else {                             // j == n-1: [N,W,C,S], CSR-loop order
                        sum = fma(v[0], xn[h], 0.0);
                        sum = fma(v[1], xw[h], sum);
                        sum = fma(v[2], xc[h], sum);
                        sum = fma(v[3], xs[h], sum);
                    }
                    if (kDot) dot_acc = fma(xc[h], sum, dot_acc);
                    if constexpr (kCheb) {
                        const long long lr = (long long)li * n + j;
                        const double t = fma(-1.0, sum, cr[h]);
                        const double u = cdv[h] * t;
                        const double dn = fma(step.g, u, step.h * cd[h]);
                        const double zn = xc[h] + dn;
                        __builtin_nontemporal_store(dn, step.d + lr);
                        step.z_out[lr] = zn;  // plain: the next step's neighbour loads re-use these lines
                        if (step.last) dot_acc = fma(cr[h], zn, dot_acc);
                    } else if (kInit) {
                        const long long lr = (long long)li * n + j;
                        const double rv = fma(-1.0, alpha * sum, bv[h]);
                        if (res.r != nullptr) __builtin_nontemporal_store(rv, res.r + lr);  // null: r0 is stored once, as p0
                        res.p[lr] = rv;  // plain: the next SpMV's neighbour loads re-use these lines
                        dot_acc = fma(rv, rv, dot_acc);
                    } else {
                        __builtin_nontemporal_store(alpha * sum, y + ((long long)li * n + j));
                    }
                }
            }
        };
        if constexpr (kSym) {
            // the tile's class (requested by the caller next to the skip flag; the same value in every lane) is looked at here for
            // the first time: the x loads, which do not depend on it, are out. A uniform tile loads no coefficient and keeps no LDS copy of E.
            if (__builtin_amdgcn_readfirstlane(tile_class) != 0) {
                if (skip != 0) return false;
                finish(std::true_type{});
            } else {
                const long long r0 = (long long)li * n + j0 + lane;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    ce[h] = d2{0.0, 0.0};
                    cs[h] = cn[h] = 0.0;
                    if (j0 + lane + 64 * h < n) {
                        ce[h] = __builtin_nontemporal_load(reinterpret_cast<const d2*>(sp.ce) + r0 + 64 * h);
                        cs[h] = sp.s[r0 + 64 * h];
                        cn[h] = sp.s[r0 + 64 * h - n];  // local grid row 0: the halo row in front of the plane
                    }
                }
                if (lane == 0 && j0 > 0) cw = sp.ce[2 * (r0 - 1) + 1];
                if (skip != 0) return false;
                finish(std::false_type{});
            }
        } else {
            if (skip != 0) return false;
            finish(std::false_type{});
        }
    } else {
        // first / last grid row of the whole grid: every row the reference's way
        if (skip != 0) return false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + lane + 64 * h;
            if (j < n) {
                const long long lr = (long long)li * n + j;
                const double sum = row_reference<false>(m, x, (int)lr, gi, j);
                if (kDot) dot_acc = fma(x[lr], sum, dot_acc);
                if constexpr (kCheb) {
                    const double rl = step.r[lr];
                    const double t = fma(-1.0, sum, rl);
                    const double u = step.dinv[lr] * t;
                    const double dn = fma(step.g, u, step.h * step.d[lr]);
                    const double zn = x[lr] + dn;
                    step.d[lr] = dn;
                    step.z_out[lr] = zn;
                    if (step.last) dot_acc = fma(rl, zn, dot_acc);
                } else if (kInit) {
                    const double rv = fma(-1.0, alpha * sum, res.b[lr]);
                    if (res.r != nullptr) res.r[lr] = rv;
                    res.p[lr] = rv;
                    dot_acc = fma(rv, rv, dot_acc);
                } else {
                    y[lr] = alpha * sum;
                }
            }
        }
    }
    if (kDot || kInit || kCheb) dot_acc = wave_sum(dot_acc);
    *dot = dot_acc;  // lane 0 holds the tile's partial
    return true;
}

// The class of the tile at (local grid row li, column tile col_tile): 1 = uniform (kernels.hpp, SymPlanes). One load per wave from
// a wave-uniform address, indexed by the tile's real position in the slab (not the launch's tile number: launches over separate
// grid rows and reversed sweeps see the same map). A byte load is a VECTOR-memory load on this part, and that is wanted: vector
// loads return in order, so the tile's x loads can be issued behind it and the wave waits for this byte alone when it tests the
// class (rowlds_tile makes the value a scalar there); a scalar load could only be waited for together with everything else the
// scalar path has in flight, in front of the first x load. No map = every tile streams the planes.
__device__ __forceinline__ int rowlds_tile_class(const SymPlanes& sp, int li, int col_tiles, int col_tile) {
    return sp.cls != nullptr ? (int)sp.cls[li * col_tiles + col_tile] : 0;
}

// Tile of workgroup b in XCD runs of `run` tiles (xcd_run_tile, stencil_row_device.hpp); tiles past `total` do not exist (-1).
__device__ __forceinline__ int rowlds_tile_of_block(int b, int run, int total, int reverse) {
    const int tile = xcd_run_tile<int>(b, run);
    if (tile >= total) return -1;
    return reverse ? total - 1 - tile : tile;  // same tiles, same partial slots, walked from the end
}

}  // namespace spmv_amd
