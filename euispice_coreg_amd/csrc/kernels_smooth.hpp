// NaN-aware separable smoothing (normalised convolution; the rule and the geometry: smooth_plan.hpp).
// Two passes, float64 throughout, no atomics, the taps of a pixel added in rising k whatever the launch:
//   k_smooth_rows  reads the stored pixels (float32 or float64), m = isfinite(v), z = m ? v : 0, and writes the planes
//                  num = C_x(z), den = C_x(m).  A work item is one segment of one row: z and m of the segment and its halo
//                  stand in LDS (taps outside the image: z = m = 0), thread t adds the taps of pixel t.
//   k_smooth_cols  reads num and den and writes out = C_y(num) / C_y(den) where the source pixel is finite and the
//                  denominator positive, NaN elsewhere.  A work item is a tile of 16 columns x 64 rows with its halo in LDS;
//                  the 32 lanes an LDS read serves together hold two neighbouring rows of 16 columns: 64 dwords, one per
//                  bank.  `out` may be the source image (float64): a pixel of it is read and written by one thread only.
// Workgroups loop over the work items (grid-stride), so no image size meets a grid limit; pixel indices are 64-bit.
#pragma once
#include "smooth_plan.hpp"

namespace coreg {

template <typename T>
__global__ __launch_bounds__(kSmoothThreads) void k_smooth_rows(const T* __restrict__ src, SmoothGeom g, SmoothTable tx,
                                                                 double* __restrict__ num, double* __restrict__ den) {
    __shared__ double z[kSmoothSeg + 2 * kSmoothMaxR];
    __shared__ double m[kSmoothSeg + 2 * kSmoothMaxR];
    const int t = (int)threadIdx.x;
    const int n_stage = kSmoothSeg + 2 * g.rx;
    for (long long item = blockIdx.x; item < g.row_items; item += gridDim.x) {
        int row, col;
        const bool live = smooth_row_pixel(g, item, t, &row, &col);
        const long long c0 = (long long)smooth_row_x0(g, item) - g.rx;  // column of z[0]
        const long long base = (long long)row * g.W;
        for (int e = t; e < n_stage; e += kSmoothThreads) {
            const long long c = c0 + e;
            double v = 0.0, f = 0.0;
            if (c >= 0 && c < g.W) {
                const double p = (double)src[base + c];
                if (isfinite(p)) {
                    v = p;
                    f = 1.0;
                }
            }
            z[e] = v;
            m[e] = f;
        }
        __syncthreads();
        if (live) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < tx.n; ++k) {
                const double w = tx.w[k];
                a = fma(w, z[t + k], a);
                b = fma(w, m[t + k], b);
            }
            num[base + col] = a;
            den[base + col] = b;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(kSmoothThreads) void k_smooth_cols(const T* src, SmoothGeom g, SmoothTable ty,
                                                                 const double* __restrict__ num,
                                                                 const double* __restrict__ den, double* out) {
    extern __shared__ double smooth_lds[];
    const int t = (int)threadIdx.x;
    const int n_rows = kSmoothColH + 2 * g.ry;  // rows staged: the tile and its halo
    double* sn = smooth_lds;
    double* sd = smooth_lds + (size_t)n_rows * kSmoothColW;
    for (long long item = blockIdx.x; item < g.col_items; item += gridDim.x) {
        int y0, x0;
        smooth_col_origin(g, item, &y0, &x0);
        for (int e = t; e < n_rows * kSmoothColW; e += kSmoothThreads) {
            const long long y = (long long)y0 - g.ry + e / kSmoothColW, x = (long long)x0 + e % kSmoothColW;
            double a = 0.0, b = 0.0;
            if (y >= 0 && y < g.H && x < g.W) {
                const long long q = y * g.W + x;
                a = num[q];
                b = den[q];
            }
            sn[e] = a;
            sd[e] = b;
        }
        __syncthreads();
        for (int q = 0; q < kSmoothColQ; ++q) {
            int row, col;
            if (!smooth_col_pixel(g, item, t, q, &row, &col)) continue;
            const int first = smooth_col_tile_row(t, q) * kSmoothColW + t % kSmoothColW;  // tap 0: tile row - ry, staged at row
            double a = 0.0, b = 0.0;
            for (int k = 0; k < ty.n; ++k) {
                const double w = ty.w[k];
                a = fma(w, sn[first + k * kSmoothColW], a);
                b = fma(w, sd[first + k * kSmoothColW], b);
            }
            const long long p = (long long)row * g.W + col;
            const double v = (double)src[p];
            out[p] = (isfinite(v) && b > 0.0) ? a / b : __longlong_as_double(0x7ff8000000000000ll);
        }
        __syncthreads();
    }
}

}  // namespace coreg
