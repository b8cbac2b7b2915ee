// The plan of one NaN-aware separable smoothing (coreg_smooth_small, coreg_set_reference_smoothing, coreg_pixels_smooth_*,
// DESIGN section 8): the table checks with their code and message, and the launch geometry of the two passes -- which work
// item and thread writes which pixel.  Plain C++ with no HIP dependency: included by kernels_smooth.hpp (the kernels take
// their pixels from the functions below) and used by the host parts of libcoreg_hip.so's one translation unit;
// tests/native/smooth_rules.cpp walks it on the host under sanitizers.
//
// The rule: m = isfinite(v), z = where(m, v, 0); num = C_y(C_x(z)), den = C_y(C_x(m)), C_x(a)[j,i] = sum_k wx[k] a[j, i+k-rx]
// in rising k (taps outside the image add nothing), C_y alike along y; out = num / den where m and den > 0, else NaN.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/coreg_hip.h"

#if defined(__HIPCC__)
#define COREG_SM_HD __host__ __device__ __forceinline__
#else
#define COREG_SM_HD inline
#endif

namespace coreg {

constexpr int kSmoothMaxR = 64;                      // taps reach this far to either side at most
constexpr int kSmoothMaxTaps = 2 * kSmoothMaxR + 1;  // entries of a table at most
constexpr int kSmoothThreads = 256;                  // threads of a work item, both passes
constexpr int kSmoothSeg = 256;   // row pass: a work item is kSmoothSeg pixels of one row, one per thread
constexpr int kSmoothColW = 16;   // column pass: a work item is a tile of kSmoothColW columns (128 bytes of a float64 row)
constexpr int kSmoothColH = 64;   //              x kSmoothColH rows: thread t has column t % 16 and rows t / 16 + 16 q
constexpr int kSmoothColQ = kSmoothColH / (kSmoothThreads / kSmoothColW);  // rows per thread (q = 0..3)
constexpr long long kSmoothMaxGrid = 65536;  // workgroups of a launch at most: each loops over its work items
static_assert(kSmoothSeg == kSmoothThreads && kSmoothColQ * (kSmoothThreads / kSmoothColW) == kSmoothColH, "geometry");

// one table as a kernel argument (the taps are read with a wave-uniform index)
struct SmoothTable {
    double w[kSmoothMaxTaps];
    int n;  // entries: 2 r + 1
    int r;
};

// nullptr: the table is good; else what is wrong with it (COREG_EINVAL)
inline const char* smooth_table_refusal(const double* w, long long n) {
    if (!w) return "smoothing: null table";
    if (n < 1 || n > kSmoothMaxTaps || n % 2 == 0) return "smoothing: a table needs an odd number of entries from 1 to 129";
    double sum = 0.0;
    for (long long k = 0; k < n; ++k) {
        if (!std::isfinite(w[k])) return "smoothing: a table entry is not finite";
        if (w[k] < 0.0) return "smoothing: a table entry is negative";
        sum += w[k];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return "smoothing: the entries of a table must have a positive, finite sum";
    return nullptr;
}

inline void smooth_table_fill(SmoothTable* t, const double* w, int n) {
    for (int k = 0; k < kSmoothMaxTaps; ++k) t->w[k] = k < n ? w[k] : 0.0;
    t->n = n;
    t->r = n / 2;
}

// ---- geometry: shared by the kernels and the host ------------------------------------------------------------------------
struct SmoothGeom {
    int W, H;             // the image
    int rx, ry;           // reach of the x / y table
    int n_seg;            // row pass: segments per row
    int n_tx, n_ty;       // column pass: tiles per row of tiles, rows of tiles
    long long row_items;  // H x n_seg
    long long col_items;  // n_ty x n_tx
};

// row pass: the pixel thread t of work item `item` writes; false: none (past the end of the row; *col = W then).
// (sums of a coordinate and an offset are 64-bit throughout: a row or column may have close to 2^31 pixels)
COREG_SM_HD bool smooth_row_pixel(const SmoothGeom& g, long long item, int t, int* row, int* col) {
    *row = (int)(item / g.n_seg);
    const long long c = (item % g.n_seg) * kSmoothSeg + t;
    *col = (int)(c < g.W ? c : g.W);
    return c < g.W;
}
// ... and the first column of the item's segment
COREG_SM_HD int smooth_row_x0(const SmoothGeom& g, long long item) { return (int)(item % g.n_seg) * kSmoothSeg; }

// column pass: the first row / column of the item's tile
COREG_SM_HD void smooth_col_origin(const SmoothGeom& g, long long item, int* y0, int* x0) {
    *y0 = (int)(item / g.n_tx) * kSmoothColH;
    *x0 = (int)(item % g.n_tx) * kSmoothColW;
}
// the row of the tile thread t writes at its q-th turn (neighbouring threads of a wave: neighbouring rows)
COREG_SM_HD int smooth_col_tile_row(int t, int q) { return t / kSmoothColW + (kSmoothThreads / kSmoothColW) * q; }
// the pixel thread t of work item `item` writes at its q-th turn; false: none (outside the image)
COREG_SM_HD bool smooth_col_pixel(const SmoothGeom& g, long long item, int t, int q, int* row, int* col) {
    int y0, x0;
    smooth_col_origin(g, item, &y0, &x0);
    const long long r = (long long)y0 + smooth_col_tile_row(t, q), c = (long long)x0 + t % kSmoothColW;
    *row = (int)(r < g.H ? r : g.H);
    *col = (int)(c < g.W ? c : g.W);
    return r < g.H && c < g.W;
}

// bytes of LDS of a work item: the row pass stages z and m of a segment and its halo, the column pass num and den of a tile
// and its halo (at r = 64: 6 KiB and 48 KiB, so that three column items share a compute unit's 160 KiB)
inline size_t smooth_row_lds_bytes() { return (size_t)2 * (kSmoothSeg + 2 * kSmoothMaxR) * sizeof(double); }
inline size_t smooth_col_lds_bytes(int ry) { return (size_t)2 * (kSmoothColH + 2 * ry) * kSmoothColW * sizeof(double); }

// A refusal (code != COREG_OK, msg) or what the two launches need
struct SmoothPlan {
    int code = COREG_OK;
    const char* msg = nullptr;
    SmoothGeom g = {};
    unsigned row_grid = 0, col_grid = 0;  // workgroups: min(items, kSmoothMaxGrid)
    size_t col_lds = 0;                   // dynamic LDS of the column pass
};

inline SmoothPlan smooth_plan(long long H, long long W, const double* wy, long long n_wy, const double* wx, long long n_wx) {
    SmoothPlan p;
    const char* why = smooth_table_refusal(wy, n_wy);
    if (!why) why = smooth_table_refusal(wx, n_wx);
    if (!why && (H < 1 || W < 1 || H * W > 2147483647ll)) why = "smoothing: empty image, or more than 2^31 - 1 pixels";
    if (why) {
        p.code = COREG_EINVAL;
        p.msg = why;
        return p;
    }
    SmoothGeom& g = p.g;
    g.W = (int)W;
    g.H = (int)H;
    g.rx = (int)(n_wx / 2);
    g.ry = (int)(n_wy / 2);
    g.n_seg = (int)((W + kSmoothSeg - 1) / kSmoothSeg);  // (64-bit: W + 255 may pass 2^31)
    g.n_tx = (int)((W + kSmoothColW - 1) / kSmoothColW);
    g.n_ty = (int)((H + kSmoothColH - 1) / kSmoothColH);
    g.row_items = (long long)g.H * g.n_seg;
    g.col_items = (long long)g.n_ty * g.n_tx;
    p.row_grid = (unsigned)std::min(g.row_items, kSmoothMaxGrid);
    p.col_grid = (unsigned)std::min(g.col_items, kSmoothMaxGrid);
    p.col_lds = smooth_col_lds_bytes(g.ry);
    return p;
}

}  // namespace coreg
