// Part of csrc/kernels.hpp: the integer pixel-lag sweep (pxlshift.AlignmentPixels).
//
//   k_pixels_resample<MODE>   order-1 map_coordinates(mode='constant', prefilter=False) of a float64 image at an affine
//                             (sub-resolution, identity, displacement) or polar (rotation plane) coordinate rule; a
//                             sample outside the image, and every value equal to the fill, becomes NaN
//   k_pixels_sweep<PASS>      one workgroup per (rotation plane, dy, group of <= 16 dx lags within 16 columns): pass 0
//                             leaves n, sum a, sum b of the kept pixels per lag, pass 1 the centred sums about the
//                             means of pass 0.  Passes kPixR0 / kPixR1 are the same walk for residus_masked, the
//                             np.std of d = (b - a) / sqrt(b) over isfinite(a) & isfinite(b) (b: the large image, the
//                             reference): R0 leaves n of the finite terms, sum d and the number of kept terms that are
//                             not finite (b <= 0: "poisoned", DESIGN Q23), R1 the squares about the mean of R0; the
//                             band's sqrt(b) is taken once per staged box pixel, in a second LDS plane these two passes
//                             alone declare.  No atomics, no accumulation across workgroups: the sums of a lag depend
//                             on the lag alone, not on the group it runs in
//   k_pixels_sweep_tiles<PASS> the same four passes per tile of the small-image plane (the local shift field): one
//                             workgroup per (group, dy, rotation plane x tile) walks the tile's rectangle alone; the body
//                             is the one text of csrc/kernels_pixels_sweep_body.hpp, included in either kernel.  The
//                             tiles may overlap: their origins are multiples of a step (PixStep), the tile shape or less
//   k_pixels_finalize         correlation: float32-rounded numerator / sqrt(product of the centred squares), NaN for an
//                             empty or flat overlap; residus_masked: sqrt(sum of squares / n), NaN for no finite term
//                             or a poisoned one; either way the lag's sample count
//   k_pixels_destretch<T>     the resample of a cube [n_planes][ny][nx] of stored type T (float / double) by a local shift
//                             field (csrc/pixels_field.hpp): one thread per output pixel forms
//                             the displacement, the taps and the weights once and walks a chunk of planes with them
//
// The constants of the band and the groups (kPixG, kPixTile, kPixBandRows, kPixLdsB, ...) and the PODs PixGroup, PixTiles,
// PixStep are declared in csrc/pixels_plan.hpp, with the host's planner that forms groups and band and checks them
// against these bounds.
//
// Reference arithmetic restated (paths relative to euispice_coreg/): pxlshift/alignment_pixels.py:38-55 (mask),
// pxlshift/c_correlate.py:41-63 (Pearson, numerator stored as float32), :126-143 (sub-resolution), :72-81 +
// utils/matrix_transform.py:78-106 (polar round trip), :86-107 (displacement of the large image).
#pragma once
#include "pixels_field.hpp"
#include "pixels_plan.hpp"  // kPixG ... kPixR1, PixGroup, PixTiles, PixStep: what the kernels share with the host's planner
namespace coreg {

enum { PIX_AFFINE = 0, PIX_POLAR = 1 };

struct PixResample {
    const double* src;  // [sH][sW]
    double* dst;        // [dH][dW]: destination pixel (j, i) is sample (j0 + j, i0 + i) of the rule
    int sW, sH, dW, dH, i0, j0;
    double ax, bx, ay, by;  // affine: x = i * ax + bx, y = j * ay + by
    double xc, yc, drot;    // polar: rotation by drot [rad] about (xc, yc)
    double fill;
};

// scipy's order-1 sample, products and additions in ni_interpolation.c's order ((pixel * wy) * wx, taps row by row, summed
// from 0), so that an unrotated sample equals the reference's to the bit.  A tap one past the last pixel (coordinate
// exactly n - 1, weight 0) is the mirrored pixel n - 2, through which a NaN still propagates.
__device__ __forceinline__ double pixels_sample(const double* __restrict__ img, int W, int H, double x, double y, double fill) {
#pragma clang fp contract(off)
    if (!((x >= 0.0) & (x <= (double)(W - 1)) & (y >= 0.0) & (y <= (double)(H - 1)))) return fill;
    const double fx = floor(x), fy = floor(y);
    const double tx = x - fx, ty = y - fy;
    const double wx[2] = {1.0 - tx, tx}, wy[2] = {1.0 - ty, ty};
    const int x0 = (int)fx, y0 = (int)fy;
    const int xs[2] = {x0, x0 + 1 < W ? x0 + 1 : (W > 1 ? W - 2 : 0)};
    const int ys[2] = {y0, y0 + 1 < H ? y0 + 1 : (H > 1 ? H - 2 : 0)};
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            double c = img[(size_t)ys[a] * W + xs[b]];
            c = c * wy[a];
            c = c * wx[b];
            t = t + c;
        }
    return t;
}

template <int MODE>
__global__ __launch_bounds__(kPixThreads) void k_pixels_resample(PixResample p) {
#pragma clang fp contract(off)
    const long long n = (long long)p.dW * p.dH;
    for (long long q = (long long)blockIdx.x * kPixThreads + threadIdx.x; q < n; q += (long long)gridDim.x * kPixThreads) {
        const int j = (int)(q / p.dW), i = (int)(q - (long long)j * p.dW);
        const double gi = (double)(p.i0 + i), gj = (double)(p.j0 + j);
        double x, y;
        if (MODE == PIX_AFFINE) {
            x = gi * p.ax + p.bx;
            y = gj * p.ay + p.by;
        } else {
            const double ddx = gi - p.xc, ddy = gj - p.yc;
            const double r = sqrt(ddx * ddx + ddy * ddy);
            const double th = atan2(ddy, ddx) + p.drot;
            x = r * cos(th) + p.xc;
            y = r * sin(th) + p.yc;
        }
        const double v = pixels_sample(p.src, p.sW, p.sH, x, y, p.fill);
        p.dst[q] = v == p.fill ? __builtin_nan("") : v;
    }
}

struct PixSweep {
    const double* planes;  // [n_rot][h][w]
    const double* box;     // [bH][bW]: the sub-resolved large image from (slice origin + min lag) on
    const PixGroup* groups;
    const int* lag_dx;
    const int* lag_dy;
    const double* sums0;   // pass 1 / R1 reads: [n_rot][n_dy][n_dx][3] = n, sum a, sum b / n finite, sum d, n poisoned
    double* sums;          // the pass's output, same layout
    int w, h, bW, bH, n_dx, n_dy, min_dx, min_dy;
    int cw, bh;            // band: columns [c0, c0 + cw) x rows [r0, r0 + bh), cw * bh <= kPixTile, bh <= kPixBandRows
};

template <int PASS>
__global__ __launch_bounds__(kPixThreads) void k_pixels_sweep(PixSweep p) {
    constexpr bool TILED = false;
    const PixTiles t = {0, 0, 1, 1, 0};  // (never read: every use sits behind TILED)
    const PixStep st = {0, 0};           // (likewise)
#include "kernels_pixels_sweep_body.hpp"
}

// The same walk per tile: one workgroup per (group of dx lags, dy, rotation plane x tile), blockIdx.z = kr * n_tiles + tile.
// Sums [n_tiles][n_rot][n_dy][n_dx][3]; pass 1 / R1 centre about the tile's own means of pass 0 / R0.  The band (p.cw, p.bh)
// is that of the nominal tile shape, one value for the launch; a tile's sums depend on the tile and the lag alone.
template <int PASS>
__global__ __launch_bounds__(kPixThreads) void k_pixels_sweep_tiles(PixSweep p, PixTiles t, PixStep st) {
    constexpr bool TILED = true;
#include "kernels_pixels_sweep_body.hpp"
}

// corr[(i * n_dy + j) * n_rot + k] and counts[...] from the sums of lag (k, j, i); resid: the residus_masked score.
// gridDim.y tiles, each with sums and a cube of its own one after the other (1: the untiled sweep)
__global__ __launch_bounds__(kPixThreads) void k_pixels_finalize(const double* __restrict__ sums0, const double* __restrict__ sums1,
                                                                  int n_dx, int n_dy, int n_rot, int resid,
                                                                  double* __restrict__ corr, double* __restrict__ counts) {
    const long long n = (long long)n_dx * n_dy * n_rot;
    const long long q = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (q >= n) return;
    const int i = (int)(q % n_dx), j = (int)((q / n_dx) % n_dy), k = (int)(q / ((long long)n_dx * n_dy));
    const long long tile0 = (long long)blockIdx.y * n;  // (a tiled sweep: one cube per tile, blockIdx.y the tile)
    sums0 += 3 * tile0;
    sums1 += 3 * tile0;
    corr += tile0;
    counts += tile0;
    const double cnt = sums0[3 * q];
    double r = __builtin_nan("");
    if (!resid) {
        const double num = sums1[3 * q], va = sums1[3 * q + 1], vb = sums1[3 * q + 2];
        if (cnt > 0.0 && va != 0.0 && vb != 0.0) r = (double)(float)num / sqrt(va * vb);
    } else {
        // np.std of the kept terms: NaN when one of them is not finite (sums0's third entry counts those)
        if (cnt > 0.0 && sums0[3 * q + 2] == 0.0) r = sqrt(sums1[3 * q] / cnt);
    }
    const long long o = ((long long)i * n_dy + j) * n_rot + k;
    corr[o] = r;
    counts[o] = cnt;
}

// Destretch: dst[p][Y][X] = order-1 sample of src[p] at (Y - v, X - u), (u, v) the field's displacement at (Y, X); no
// sample (NaN) outside the plane.  blockIdx.x deals runs of kPixThreads output pixels (consecutive along X: the stores and,
// the displacement being smooth, the tap rows are coalesced), blockIdx.y chunks of kPixDsPlanes planes (the last one
// short; a grid stride when there are more chunks than gridDim.y).  The node arrays are a few hundred doubles at most
// and are read through the cache.  disp: nullptr or [2][ny][nx], (u, v) of every pixel, stored by the first chunk.
constexpr int kPixDsPlanes = 8;

struct PixDestretch {
    const void* src;  // [n_planes][ny][nx] of T
    void* dst;        // the same
    double* disp;
    PixField f;
    int nx, ny, n_planes;
};

template <class T>
__global__ __launch_bounds__(kPixThreads) void k_pixels_destretch(PixDestretch p) {
#pragma clang fp contract(off)
    const long long n = (long long)p.nx * p.ny;
    const long long q = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (q >= n) return;
    const int Y = (int)(q / p.nx), X = (int)(q - (long long)Y * p.nx);
    double u, v;
    field_displacement(p.f, (double)X, (double)Y, &u, &v);
    if (p.disp && blockIdx.y == 0) {
        p.disp[q] = u;
        p.disp[n + q] = v;
    }
    const PixTaps t = field_taps(p.nx, p.ny, (double)X - u, (double)Y - v);
    const T* __restrict__ src = (const T*)p.src;
    T* __restrict__ dst = (T*)p.dst;
    for (long long p0 = (long long)blockIdx.y * kPixDsPlanes; p0 < p.n_planes; p0 += (long long)gridDim.y * kPixDsPlanes) {
        const int np = (int)(p.n_planes - p0 < kPixDsPlanes ? p.n_planes - p0 : kPixDsPlanes);
        for (int k = 0; k < np; ++k) {
            const size_t o = (size_t)(p0 + k) * (size_t)n;
            dst[o + q] = t.inside ? (T)field_sample(src + o, p.nx, t) : (T)__builtin_nan("");
        }
    }
}

}  // namespace coreg
