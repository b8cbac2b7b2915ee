// Part of csrc/kernels.hpp: the apodized windows of the local shift field (pxlshift find_local_shifts(apodization=...),
// DESIGN section 9a row P14): local correlation tracking, a weighted Pearson coefficient per (window, lag).
//
//   k_pixels_lct<PASS>      one workgroup per (group of <= 16 dx lags, dy, rotation plane x window) -- the mapping, box,
//                           planes, groups and bands of k_pixels_sweep_tiles -- with a body of its own: pixel (y, x) of the
//                           window at (r_lo, c_lo) has the weight w = wy[y - r_lo] * wx[x - c_lo], one IEEE product of two
//                           table entries (a ragged window reads the head of the tables).  Pass 0 leaves n, W = sum w,
//                           sum w a, sum w b of the kept pixels per (window, lag), pass 1 the weighted centred sums about
//                           the means sum w a / W, sum w b / W of pass 0.  n is counted in an integer register per slot
//                           (exact, and half the registers of a fourth float64 sum): pass 0 holds 16 x (3 float64 + 1
//                           int32), pass 1 the 16 x 3 sums and 16 x 2 means of k_pixels_sweep<1>.  The two table entries of
//                           a pixel are read once per staged pixel, outside the loop over the slots, straight from memory:
//                           th + tw doubles that every workgroup reads, against 16 lag slots of LDS reads and float64
//                           arithmetic per pixel; a third LDS plane would cost 16 KiB a workgroup for the same product.
//                           No atomics, no accumulation across workgroups; lanes, then waves, in a fixed order: the sums
//                           of a (window, lag) depend on the window and the lag alone
//   k_pixels_lct_finalize   corr = float32-rounded numerator / sqrt(product of the weighted centred squares), NaN when
//                           W = 0 or a variance is 0; counts = n, whatever the weights; weights = W
#pragma once
namespace coreg {

// the two weight tables of a launch: wy[th], wx[tw], finite and >= 0 (checked on the host)
struct PixWindow {
    const double* wy;
    const double* wx;
};

// (contraction off: the weight is the rounded product itself, whatever it is multiplied with or added to afterwards)
__device__ __forceinline__ double pixels_lct_weight(double wy, double wx) {
#pragma clang fp contract(off)
    return wy * wx;
}

template <int PASS>
__global__ __launch_bounds__(kPixThreads) void k_pixels_lct(PixSweep p, PixTiles t, PixStep st, PixWindow win) {
    constexpr int NS = PASS == 0 ? 4 : 3;  // sums per (window, lag) this pass leaves
    __shared__ double lds_a[kPixTile];
    __shared__ double lds_b[kPixLdsB];
    __shared__ double lds_red[kPixThreads / 64][NS * kPixG];
    const int tid = threadIdx.x;
    const PixGroup g = p.groups[blockIdx.x];
    const int jy = blockIdx.y, kr = (int)blockIdx.z / t.n_tiles;
    const int row_off = p.lag_dy[jy] - p.min_dy;  // box row of the window's first row
    const int col_off = g.dx_min - p.min_dx;      // box column of the group's first window's first column
    const int tile = (int)blockIdx.z - kr * t.n_tiles;
    const long long lag0 = (((long long)tile * t.n_rot + kr) * p.n_dy + jy) * p.n_dx + g.first;
    const int ty = tile / t.n_tx, tx = tile - ty * t.n_tx;
    const int r_lo = ty * st.sy, r_hi = min(p.h, r_lo + t.th);
    const int c_lo = tx * st.sx, c_hi = min(p.w, c_lo + t.tw);
    const double* plane = p.planes + (size_t)kr * p.w * p.h;

    int off[kPixG];
    double ma[kPixG], mb[kPixG];
#pragma unroll
    for (int s = 0; s < kPixG; ++s) {
        const bool used = s < g.count;
        off[s] = used ? p.lag_dx[g.first + s] - g.dx_min : 0;
        ma[s] = mb[s] = 0.0;
        if (PASS == 1 && used) {
            const double* s0 = p.sums0 + 4 * (lag0 + s);
            ma[s] = s0[2] / s0[1];  // (W = 0: NaN sums, and the finalize step's NaN)
            mb[s] = s0[3] / s0[1];
        }
    }
    int accn[kPixG];
    double acc0[kPixG], acc1[kPixG], acc2[kPixG];
#pragma unroll
    for (int s = 0; s < kPixG; ++s) {
        accn[s] = 0;
        acc0[s] = acc1[s] = acc2[s] = 0.0;
    }

    for (int r0 = r_lo; r0 < r_hi; r0 += p.bh) {
        const int nr = min(p.bh, r_hi - r0);
        for (int c0 = c_lo; c0 < c_hi; c0 += p.cw) {
            const int nc = min(p.cw, c_hi - c0);
            const int ncb = nc + kPixG - 1;
            __syncthreads();  // the previous band has been read
            for (int q = tid; q < nr * nc; q += kPixThreads) {
                const int r = q / nc, c = q - r * nc;
                lds_a[q] = plane[(size_t)(r0 + r) * p.w + c0 + c];
            }
            for (int q = tid; q < nr * ncb; q += kPixThreads) {
                const int r = q / ncb, c = q - r * ncb;
                const int bc = col_off + c0 + c;  // (columns past the box belong to unused slots only)
                lds_b[q] = bc < p.bW ? p.box[(size_t)(row_off + r0 + r) * p.bW + bc] : 0.0;
            }
            __syncthreads();
            for (int q = tid; q < nr * nc; q += kPixThreads) {
                const int r = q / nc, c = q - r * nc;
                const double a = lds_a[q];
                const double* brow = lds_b + r * ncb + c;
                // rows r0 - r_lo + r < th and columns c0 - c_lo + c < tw of the tables: inside the nominal window
                const double w = pixels_lct_weight(win.wy[r0 - r_lo + r], win.wx[c0 - c_lo + c]);
                const bool a_ok = a == a;
                const double wa = w * a;
#pragma unroll
                for (int s = 0; s < kPixG; ++s) {
                    const double b = brow[off[s]];
                    const bool keep = a_ok & (b == b);
                    if (PASS == 0) {
                        accn[s] += keep ? 1 : 0;
                        acc0[s] += keep ? w : 0.0;
                        acc1[s] += keep ? wa : 0.0;
                        acc2[s] += keep ? w * b : 0.0;
                    } else {
                        const double da = a - ma[s], db = b - mb[s];
                        const double wda = w * da, wdb = w * db;
                        acc0[s] += keep ? wda * db : 0.0;
                        acc1[s] += keep ? wda * da : 0.0;
                        acc2[s] += keep ? wdb * db : 0.0;
                    }
                }
            }
        }
    }
    // lanes of a wave, then the four waves in a fixed order (a count is exact in float64)
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < kPixG; ++s) {
        double v0 = acc0[s], v1 = acc1[s], v2 = acc2[s], vn = (double)accn[s];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v0 += __shfl_down(v0, d, 64);
            v1 += __shfl_down(v1, d, 64);
            v2 += __shfl_down(v2, d, 64);
            if (PASS == 0) vn += __shfl_down(vn, d, 64);
        }
        if (lane == 0) {
            if (PASS == 0) {
                lds_red[wave][NS * s + 0] = vn;
                lds_red[wave][NS * s + 1] = v0;
                lds_red[wave][NS * s + 2] = v1;
                lds_red[wave][NS * s + 3] = v2;
            } else {
                lds_red[wave][NS * s + 0] = v0;
                lds_red[wave][NS * s + 1] = v1;
                lds_red[wave][NS * s + 2] = v2;
            }
        }
    }
    __syncthreads();
    if (tid < NS * g.count) {
        double v = lds_red[0][tid];
#pragma unroll
        for (int k = 1; k < kPixThreads / 64; ++k) v += lds_red[k][tid];
        p.sums[NS * lag0 + tid] = v;
    }
}

// corr, counts and weights [(window)][(i * n_dy + j) * n_rot + k] from the sums of (window, lag (k, j, i)): sums0
// [n_windows][n_rot][n_dy][n_dx][4] = n, W, sum w a, sum w b, sums1 [...][3] = the weighted centred sums.  blockIdx.y the
// window
__global__ __launch_bounds__(kPixThreads) void k_pixels_lct_finalize(const double* __restrict__ sums0,
                                                                      const double* __restrict__ sums1, int n_dx, int n_dy,
                                                                      int n_rot, double* __restrict__ corr,
                                                                      double* __restrict__ counts, double* __restrict__ weights) {
    const long long n = (long long)n_dx * n_dy * n_rot;
    const long long q = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (q >= n) return;
    const int i = (int)(q % n_dx), j = (int)((q / n_dx) % n_dy), k = (int)(q / ((long long)n_dx * n_dy));
    const long long win0 = (long long)blockIdx.y * n;
    sums0 += 4 * win0;
    sums1 += 3 * win0;
    const double W = sums0[4 * q + 1];
    const double num = sums1[3 * q], va = sums1[3 * q + 1], vb = sums1[3 * q + 2];
    double r = __builtin_nan("");
    if (W > 0.0 && va != 0.0 && vb != 0.0) r = (double)(float)num / sqrt(va * vb);
    const long long o = win0 + ((long long)i * n_dy + j) * n_rot + k;
    corr[o] = r;
    counts[o] = sums0[4 * q];
    weights[o] = W;
}

}  // namespace coreg
