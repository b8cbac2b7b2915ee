// Part of csrc/kernels.hpp: the mutual-information score of the integer pixel-lag sweep (pxlshift method
// "mutual_information").
//
//   k_pixels_mi<TILED>   one workgroup per (group of <= 16 dx lags, dy, rotation plane [x tile]) -- the mapping, box, planes,
//                        groups and bands of k_pixels_sweep / k_pixels_sweep_tiles -- with a body of its own.  While a band
//                        is staged every pixel of the plane and of the box becomes a byte: its bin among the edges of its
//                        image (csrc/pixels_bins.hpp), or kPixBinNaN.  The workgroup keeps one joint histogram of uint32
//                        counters per lag slot in LDS, [cell][slot], and adds 1 per kept (pixel, slot): integer adds, whose
//                        result does not depend on their order (nor on the threads of the workgroup, 256 or 512).  A
//                        wave-instruction takes 4 pixels x 16 slots: the sixteen lanes of a pixel hit sixteen different
//                        histograms (neighbouring dwords), where 64 neighbouring pixels of one slot would mostly hit one
//                        counter (measured: 2.8 and 2.2 times the time at 8 and 16 bins, 1.4 times at 32).  From the
//                        finished histograms the same kernel forms the margins, the terms row by row and the score in the
//                        fixed order of pixels_bins.hpp and stores corr and counts itself: no histogram goes to memory,
//                        k_pixels_finalize is not involved.
//                        A lag's result depends on the lag (and the tile) alone, not on its slot or group.
//                        TILED: the tile's origin is (ty sy, tx sx) of the last argument, the step of the window grid
//                        (csrc/kernels_pixels.hpp: PixStep; the tile shape itself for disjoint tiles).
//
// LDS: the histograms are dynamic, kPixG * na * nb * 4 bytes (na, nb the bin counts: 64 KiB at 32 x 32, 16 KiB at 16 x 16);
// the staged bytes, edges, margins and row sums are static (about 13.5 KiB).
#pragma once
#include "pixels_bins.hpp"
namespace coreg {

constexpr int kPixMaxBins = kPixMaxEdges + 1;
// threads of a workgroup: 256, or 512 once the histograms leave room for few workgroups on a CU (above kPixMiWideBytes of
// them: 64 KiB at 32 x 32 bins is two workgroups, and two waves per SIMD do not keep the LDS busy)
constexpr int kPixMiThreads = 256, kPixMiThreadsWide = 512;
constexpr size_t kPixMiWideBytes = 16384;

struct PixBins {
    const double* edges_small;  // [n_small]
    const double* edges_large;  // [n_large]
    int n_small, n_large;
    double* corr;               // [n_tiles][n_dx][n_dy][n_rot]
    double* counts;             // the same
    int n_rot;
};

template <bool TILED, int THREADS>
__global__ __launch_bounds__(THREADS) void k_pixels_mi(PixSweep p, PixTiles t, PixBins b, PixStep st) {
    extern __shared__ uint32_t lds_hist[];  // [na * nb][kPixG]
    __shared__ double lds_edges[2][kPixMaxEdges];
    __shared__ unsigned char lds_a[kPixTile];
    __shared__ unsigned char lds_b[kPixLdsB];
    __shared__ uint32_t lds_r[kPixMaxBins][kPixG], lds_c[kPixMaxBins][kPixG], lds_n[kPixG];
    __shared__ double lds_rows[kPixMaxBins][kPixG];
    const int tid = threadIdx.x;
    const PixGroup g = p.groups[blockIdx.x];
    const int jy = blockIdx.y, kr = TILED ? (int)blockIdx.z / t.n_tiles : blockIdx.z;
    const int row_off = p.lag_dy[jy] - p.min_dy;  // box row of the window's first row
    const int col_off = g.dx_min - p.min_dx;      // box column of the group's first window's first column
    const int tile = TILED ? (int)blockIdx.z - kr * t.n_tiles : 0;
    const int ty = TILED ? tile / t.n_tx : 0, tx = TILED ? tile - ty * t.n_tx : 0;
    const int r_lo = TILED ? ty * st.sy : 0, r_hi = TILED ? min(p.h, r_lo + t.th) : p.h;
    const int c_lo = TILED ? tx * st.sx : 0, c_hi = TILED ? min(p.w, c_lo + t.tw) : p.w;
    const double* plane = p.planes + (size_t)kr * p.w * p.h;
    const int na = b.n_small + 1, nb = b.n_large + 1, n_cells = na * nb;

    for (int q = tid; q < n_cells * kPixG; q += THREADS) lds_hist[q] = 0u;
    if (tid < b.n_small) lds_edges[0][tid] = b.edges_small[tid];
    if (tid >= 64 && tid - 64 < b.n_large) lds_edges[1][tid - 64] = b.edges_large[tid - 64];

    // this thread's slot and its place among the THREADS / 16 pixels the workgroup takes per step
    const int slot = tid & (kPixG - 1), sub = tid >> 4;
    const bool used = slot < g.count;
    const int off = used ? p.lag_dx[g.first + slot] - g.dx_min : 0;

    for (int r0 = r_lo; r0 < r_hi; r0 += p.bh) {
        const int nr = min(p.bh, r_hi - r0);
        for (int c0 = c_lo; c0 < c_hi; c0 += p.cw) {
            const int nc = min(p.cw, c_hi - c0);
            const int ncb = nc + kPixG - 1;
            __syncthreads();  // the previous band has been read (the first band: the edges are in place)
            for (int q = tid; q < nr * nc; q += THREADS) {
                const int r = q / nc, c = q - r * nc;
                lds_a[q] = (unsigned char)bins_code(lds_edges[0], b.n_small, plane[(size_t)(r0 + r) * p.w + c0 + c]);
            }
            for (int q = tid; q < nr * ncb; q += THREADS) {
                const int r = q / ncb, c = q - r * ncb;
                const int bc = col_off + c0 + c;  // (columns past the box belong to unused slots only)
                lds_b[q] = bc < p.bW ? (unsigned char)bins_code(lds_edges[1], b.n_large,
                                                                 p.box[(size_t)(row_off + r0 + r) * p.bW + bc])
                                     : (unsigned char)kPixBinNaN;
            }
            __syncthreads();
            if (used) {
                // pixels q = sub, sub + step, ...: (r, c) kept by increments, no division per pixel; four pixels' bytes are
                // read before their four adds, so that the reads of one do not wait for the add of the one before
                const int step = THREADS / kPixG, dr = step / nc, dc = step - dr * nc, n_pix = nr * nc;
                int r = sub / nc, c = sub - r * nc;
                for (int q = sub; q < n_pix; q += 4 * step) {
                    int ia[4], ib[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool in = q + u * step < n_pix;
                        ia[u] = in ? lds_a[q + u * step] : kPixBinNaN;
                        ib[u] = in ? lds_b[r * ncb + c + off] : kPixBinNaN;
                        r += dr;
                        c += dc;
                        if (c >= nc) {
                            c -= nc;
                            ++r;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (ia[u] != kPixBinNaN && ib[u] != kPixBinNaN)
                            atomicAdd(&lds_hist[(ia[u] * nb + ib[u]) * kPixG + slot], 1u);
                }
            }
        }
    }
    __syncthreads();
    // margins: one thread per (row or column, slot), the slot on neighbouring lanes
    for (int q = tid; q < (na + nb) * kPixG; q += THREADS) {
        const int s = q & (kPixG - 1), k = q >> 4;
        uint32_t v = 0;
        if (k < na) {
            for (int j = 0; j < nb; ++j) v += lds_hist[(k * nb + j) * kPixG + s];
            lds_r[k][s] = v;
        } else {
            for (int i = 0; i < na; ++i) v += lds_hist[(i * nb + (k - na)) * kPixG + s];
            lds_c[k - na][s] = v;
        }
    }
    __syncthreads();
    if (tid < kPixG) {
        uint32_t v = 0;
        for (int i = 0; i < na; ++i) v += lds_r[i][tid];
        lds_n[tid] = v;
    }
    __syncthreads();
    // the terms of a row in the order of j: one thread per (row, slot)
    for (int q = tid; q < na * kPixG; q += THREADS) {
        const int s = q & (kPixG - 1), i = q >> 4;
        const uint32_t n = lds_n[s];
        lds_rows[i][s] = (s < g.count && n > 0) ? bins_mi_row(lds_hist + s, kPixG, i, nb, lds_r[i][s], &lds_c[0][s], kPixG, n) : 0.0;
    }
    __syncthreads();
    if (tid < g.count) {
        const uint32_t n = lds_n[tid];
        const long long n_lag = (long long)p.n_dx * p.n_dy * b.n_rot;
        const long long o = (long long)tile * n_lag + ((long long)(g.first + tid) * p.n_dy + jy) * b.n_rot + kr;
        b.corr[o] = bins_mi_sum(&lds_rows[0][tid], kPixG, na, n);
        b.counts[o] = (double)n;
    }
}

}  // namespace coreg
