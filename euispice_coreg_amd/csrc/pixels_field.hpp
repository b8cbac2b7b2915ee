// The destretch rule of a local shift field (pxlshift.LocalShiftField.destretch), in plain C++:
// the displacement (u, v) of a field of tile-centre nodes at an output pixel, and the four taps and weights of the
// package's order-1 sample at a coordinate.  Host- and device-callable: k_pixels_destretch (csrc/kernels_pixels.hpp)
// runs this text per thread, tests/native/fuzz_pixels_field.cpp runs it under sanitizers on the host.
//
//   D(Y, X) = S(Y - v(Y, X), X - u(Y, X)),   u = dx - rx, v = dy - ry at the tile centres
//
// Every step is one IEEE float64 operation in a fixed order, contraction off, so numpy restates it to the bit
// (tests/pxlshift_destretch_oracle.py).  No function here reads outside its arrays whatever the field or the pixel:
// a cell index lies in [0, max(n - 2, 0)], its neighbour in [0, n - 1], a tap index in [0, W - 1] x [0, H - 1].
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define COREG_PF_HD __host__ __device__ __forceinline__
#else
#define COREG_PF_HD inline
#endif

namespace coreg {

enum { PIX_FIELD_BILINEAR = 0, PIX_FIELD_NEAREST = 1 };

struct PixField {
    int n_ty, n_tx, th, tw, interp;
    const double* ys;  // [n_ty] rows of the tile centres, strictly increasing
    const double* xs;  // [n_tx] columns of the tile centres, strictly increasing
    const double* u;   // [n_ty][n_tx]
    const double* v;   // [n_ty][n_tx]
    double row_offset, col_offset;  // output pixel (Y, X) has field coordinate (Y - row_offset, X - col_offset)
};

// The cell of coordinate p on an axis of n nodes c[0] < c[1] < ...: i0 the largest index with c[i0] <= p, clamped to
// [0, n - 2]; i1 = i0 + 1; f = (p - c[i0]) / (c[i1] - c[i0]) clamped to [0, 1] (the field is held constant outside the
// outer nodes).  One node: i0 = i1 = 0, f = 0.
COREG_PF_HD void field_cell(const double* c, int n, double p, int* i0, int* i1, double* f) {
#pragma clang fp contract(off)
    if (n < 2) {
        *i0 = *i1 = 0;
        *f = 0.0;
        return;
    }
    int lo = 0, hi = n - 1;  // c[lo] <= p or lo == 0; c[hi] > p or hi == n - 1
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (c[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    double t = (p - c[lo]) / (c[lo + 1] - c[lo]);
    t = t < 0.0 ? 0.0 : t;
    t = t > 1.0 ? 1.0 : t;
    *i0 = lo;
    *i1 = lo + 1;
    *f = t;
}

// clamp(floor(p / t), 0, n - 1): the tile of size t a coordinate falls into
COREG_PF_HD int field_tile(double p, int t, int n) {
#pragma clang fp contract(off)
    const double q = floor(p / (double)t);
    if (!(q > 0.0)) return 0;
    return q < (double)(n - 1) ? (int)q : n - 1;
}

// (u, v) at output pixel (Y, X)
COREG_PF_HD void field_displacement(const PixField& f, double X, double Y, double* u, double* v) {
#pragma clang fp contract(off)
    const double xp = X - f.col_offset, yp = Y - f.row_offset;
    if (f.interp == PIX_FIELD_NEAREST) {
        const int q = field_tile(yp, f.th, f.n_ty) * f.n_tx + field_tile(xp, f.tw, f.n_tx);
        *u = f.u[q];
        *v = f.v[q];
        return;
    }
    int i0, i1, j0, j1;
    double fx, fy;
    field_cell(f.xs, f.n_tx, xp, &i0, &i1, &fx);
    field_cell(f.ys, f.n_ty, yp, &j0, &j1, &fy);
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double* a[2] = {f.u, f.v};
    double r[2];
    for (int k = 0; k < 2; ++k) {
        const double a00 = a[k][j0 * f.n_tx + i0], a01 = a[k][j0 * f.n_tx + i1];
        const double a10 = a[k][j1 * f.n_tx + i0], a11 = a[k][j1 * f.n_tx + i1];
        const double top = a00 * gx + a01 * fx, bot = a10 * gx + a11 * fx;
        r[k] = top * gy + bot * fy;
    }
    *u = r[0];
    *v = r[1];
}

// The taps of the order-1 sample at (x, y) of a W x H image, as pixels_sample forms them: outside [0, W - 1] x
// [0, H - 1] (or not a number) there is no sample; a coordinate exactly on the last pixel takes the mirrored pixel
// n - 2 at weight 0, through which a NaN still propagates.
struct PixTaps {
    int x[2], y[2];
    double wx[2], wy[2];
    bool inside;
};

COREG_PF_HD PixTaps field_taps(int W, int H, double x, double y) {
#pragma clang fp contract(off)
    PixTaps t = {{0, 0}, {0, 0}, {0.0, 0.0}, {0.0, 0.0}, false};
    if (!((x >= 0.0) & (x <= (double)(W - 1)) & (y >= 0.0) & (y <= (double)(H - 1)))) return t;
    const double fx = floor(x), fy = floor(y);
    const double tx = x - fx, ty = y - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    t.inside = true;
    t.wx[0] = 1.0 - tx;
    t.wx[1] = tx;
    t.wy[0] = 1.0 - ty;
    t.wy[1] = ty;
    t.x[0] = x0;
    t.x[1] = x0 + 1 < W ? x0 + 1 : (W > 1 ? W - 2 : 0);
    t.y[0] = y0;
    t.y[1] = y0 + 1 < H ? y0 + 1 : (H > 1 ? H - 2 : 0);
    return t;
}

// The sample of one plane [H][W] of stored type T at taps that are inside: taps row by row, (pixel * wy) * wx, summed
// from 0, in float64
template <class T>
COREG_PF_HD double field_sample(const T* img, int W, const PixTaps& t) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            double c = (double)img[(size_t)t.y[a] * W + t.x[b]];
            c = c * t.wy[a];
            c = c * t.wx[b];
            s = s + c;
        }
    return s;
}

}  // namespace coreg
