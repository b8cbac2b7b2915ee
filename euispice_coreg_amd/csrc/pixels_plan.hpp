// The plan of a pixel-lag sweep (pxlshift): every check of a request, the window grid, the dx groups, the
// band, the launch grid and the byte layout of the plan blob the kernels read.  Plain C++ with no HIP dependency: included
// by kernels_pixels.hpp (the constants and PODs the kernels share with the host) and used by host_pixels.hpp, parts of
// libcoreg_hip.so's one translation unit; tests/native/pixels_plan_rules.cpp walks it on the host under sanitizers.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/coreg_hip.h"

namespace coreg {

constexpr int kPixG = 16;         // dx lags per workgroup, all within kPixG columns of the group's first
constexpr int kPixThreads = 256;
constexpr int kPixTile = 2048;    // small-image pixels staged per band (8 per thread)
constexpr int kPixBandRows = 64;  // rows per band at most: bounds the G - 1 extra columns of the large rows
constexpr int kPixLdsB = kPixTile + kPixBandRows * (kPixG - 1);
constexpr int kPixR0 = 2, kPixR1 = 3;  // k_pixels_sweep<PASS>: the two passes of residus_masked (0 / 1: Pearson)

// One group of dx lags: entries [first, first + count) of the dx list, every one within kPixG columns of dx_min.
struct PixGroup {
    int first, count, dx_min, pad;
};

// The window grid of k_pixels_sweep_tiles: tile (ty, tx) is rows [ty sy, min(h, ty sy + th)) x columns [tx sx, min(w, tx sx + tw))
// of every plane (a rotated plane is rotated about the whole image's centre; a tile is a rectangle of it).  (sy, sx) = (th,
// tw): disjoint tiles; a smaller step: windows that overlap
struct PixTiles {
    int th, tw, n_tx, n_tiles, n_rot;
};

// The step of the grid, 1 <= sy <= th, 1 <= sx <= tw: the last argument of the kernels that can be tiled, not a part of
// PixTiles, so that the untiled k_pixels_mi finds its arguments where it found them before the step existed
struct PixStep {
    int sy, sx;
};

// What a band of cw columns x bh rows stages: the plane's pixels into kPixTile entries, the box rows, kPixG - 1 columns
// wider, into kPixLdsB (every sweep kernel's lds_b)
static_assert(kPixLdsB >= kPixTile + kPixBandRows * (kPixG - 1), "lds_b must hold a full band's box rows");
inline bool pixels_band_fits(int cw, int bh) {
    return cw >= 1 && bh >= 1 && bh <= kPixBandRows && cw * bh <= kPixTile && bh * (cw + kPixG - 1) <= kPixLdsB;
}

// windows along an axis of n pixels: one when the window covers it, else ceil((n - size) / step) + 1 (step = size:
// ceil(n / size), the disjoint tiles)
inline long long pixels_windows(int n, int size, int step) { return n <= size ? 1 : ((long long)n - size + step - 1) / step + 1; }

// (host_upload.hpp's too_many: more than 2^31 - 1 elements)
inline bool pixels_too_many(long long a, long long b) { return a * b > 2147483647ll; }

// groups: runs of the dx list, at most kPixG entries, all within kPixG columns of the run's smallest
inline std::vector<PixGroup> pixels_groups(const int32_t* lag_dx, int n_dx) {
    std::vector<PixGroup> groups;
    for (int i = 0; i < n_dx;) {
        int lo = lag_dx[i], hi = lo, n = 1;
        while (i + n < n_dx && n < kPixG) {
            const int v = lag_dx[i + n];
            if (std::max(hi, v) - std::min(lo, v) > kPixG - 1) break;
            lo = std::min(lo, v);
            hi = std::max(hi, v);
            ++n;
        }
        groups.push_back(PixGroup{i, n, lo, 0});
        i += n;
    }
    return groups;
}

// What the caller asks for.  tile: nullptr (the untiled sweep: one cube [n_dx][n_dy][n_rot]) or {rows, columns} of a tile
// (one such cube per tile, [n_ty][n_tx] of them).  step: nullptr (the tile shape: disjoint tiles) or {rows, columns}
// between the origins of neighbouring tiles.  wy, wx: both nullptr, or the weight tables [tile rows], [tile columns] of an
// apodized sweep (the correlation only: k_pixels_lct).
struct PixRequest {
    const coreg_pixels_plan* pl;
    int method;
    const int32_t *tile, *step;
    const double *wy, *wx;
    const double* out;  // (only whether it is null)
};

// The part of the handle's state the checks read
struct PixHave {
    bool large, small;    // the images are set
    int w, h;             // the small image
    int n_edges_small, n_edges_large;  // coreg_pixels_set_bins; 0: not set
};

// A refusal (code != COREG_OK, msg) or everything the launches need
struct PixPlan {
    int code = COREG_OK;
    const char* msg = nullptr;
    PixPlan() {}
    PixPlan(int refusal, const char* why) : code(refusal), msg(why) {}
    bool resid = false, mi = false, lct = false, tiled = false;
    int min_dx = 0, max_dx = 0, min_dy = 0, max_dy = 0;
    int bW = 0, bH = 0;  // the box: the part of the sub-resolved large image the lags can reach
    PixTiles tl = {};
    PixStep ts = {0, 0};
    long long n_tiles = 1, n_lag = 0, n_out = 0;
    std::vector<PixGroup> groups;
    int cw = 0, bh = 0;         // the band of the whole image, or of the nominal tile: one value for the launch
    unsigned grid[3] = {0, 0, 0};   // the sweep kernels: (groups, dy, rotation planes x tiles)
    unsigned fin_grid[2] = {0, 0};  // the finalize kernels: (lags / kPixThreads, tiles)
    // the blob: groups at 0, dx, dy, then -- on a multiple of 8 bytes -- n_a and n_b doubles: the two edge lists (mutual
    // information) or the two weight tables (an apodized sweep); neither: the blob ends behind dy
    size_t off_dx = 0, off_dy = 0, off_a = 0, off_b = 0, bytes = 0;
    int n_a = 0, n_b = 0;
};

namespace detail {
// nullptr, or what is wrong with a weight table
inline const char* pixels_weights_wrong(const double* tab, int len) {
    bool any = false;
    for (int k = 0; k < len; ++k) {
        if (!std::isfinite(tab[k]) || tab[k] < 0.0) return "pixels: a weight is negative or not finite";
        any = any || tab[k] > 0.0;
    }
    return any ? nullptr : "pixels: a weight table without a positive entry";
}
}  // namespace detail

// The checks in the order a caller sees them fail, then the plan.  No GPU work, nothing of the handle changes.
inline PixPlan pixels_plan(const PixRequest& rq, const PixHave& have) {
    const coreg_pixels_plan* pl = rq.pl;
    const int method = rq.method;
    if (method == COREG_METHOD_RESIDUS)
        return PixPlan(COREG_ENOTIMPL, "pixels: method residus is not implemented (the reference's pxlshift has no such score); "
                                       "residus_masked is");
    if (method != COREG_METHOD_CORRELATION && method != COREG_METHOD_RESIDUS_MASKED && method != COREG_METHOD_MUTUAL_INFORMATION)
        return PixPlan(COREG_EINVAL, "pixels: unknown method");
    PixPlan p;
    p.resid = method == COREG_METHOD_RESIDUS_MASKED;
    p.mi = method == COREG_METHOD_MUTUAL_INFORMATION;
    p.lct = rq.wy || rq.wx;
    p.tiled = rq.tile != nullptr;
    if (p.lct && (!rq.wy || !rq.wx || !rq.tile))
        return PixPlan(COREG_EINVAL, "pixels: an apodized sweep needs both weight tables and a tile");
    if (p.lct && method != COREG_METHOD_CORRELATION)
        return PixPlan(COREG_EINVAL, "pixels: weight tables belong to the correlation (no weighted residus_masked or histogram)");
    if (p.mi && (have.n_edges_small < 1 || have.n_edges_large < 1))
        return PixPlan(COREG_ESTATE, "pixels: mutual information needs its bins (coreg_pixels_set_bins)");
    if (!have.large || !have.small) return PixPlan(COREG_ESTATE, "pixels: the large and the small image must be set");
    if (!pl || !rq.out || !pl->lag_dx || !pl->lag_dy || !pl->lag_drot) return PixPlan(COREG_EINVAL, "pixels: null pointer");
    if (pl->n_dx < 1 || pl->n_dy < 1 || pl->n_rot < 1) return PixPlan(COREG_EINVAL, "pixels: empty lag axis");
    if (pl->n_dy > 65535 || pl->n_rot > 65535) return PixPlan(COREG_EINVAL, "pixels: more than 65535 dy or rotation lags");
    if (!(pl->ratio1 > 0.0) || !(pl->ratio2 > 0.0) || pl->sub_nx < 1 || pl->sub_ny < 1)
        return PixPlan(COREG_EINVAL, "pixels: ratios and sub-resolved shape must be positive");
    const int w = have.w, hh = have.h;
    p.n_lag = (long long)pl->n_dx * pl->n_dy * pl->n_rot;
    if (p.n_lag > (1ll << 28)) return PixPlan(COREG_EINVAL, "pixels: too many lags");
    if (p.tiled) {
        PixTiles& tl = p.tl;
        PixStep& ts = p.ts;
        if (rq.tile[0] < 1 || rq.tile[0] > hh || rq.tile[1] < 1 || rq.tile[1] > w)
            return PixPlan(COREG_EINVAL, "pixels: the tile shape must lie within [1, h] x [1, w] of the small image");
        tl.th = rq.tile[0];
        tl.tw = rq.tile[1];
        if (rq.step && (rq.step[0] < 1 || rq.step[0] > tl.th || rq.step[1] < 1 || rq.step[1] > tl.tw))
            return PixPlan(COREG_EINVAL, "pixels: the tile step must lie within [1, tile rows] x [1, tile columns]");
        ts.sy = rq.step ? rq.step[0] : tl.th;
        ts.sx = rq.step ? rq.step[1] : tl.tw;
        if (p.lct) {
            if (const char* wrong = detail::pixels_weights_wrong(rq.wy, tl.th)) return PixPlan(COREG_EINVAL, wrong);
            if (const char* wrong = detail::pixels_weights_wrong(rq.wx, tl.tw)) return PixPlan(COREG_EINVAL, wrong);
        }
        const long long n_tx = pixels_windows(w, tl.tw, ts.sx);
        p.n_tiles = pixels_windows(hh, tl.th, ts.sy) * n_tx;  // (either factor at most the axis: no overflow)
        tl.n_tx = (int)n_tx;
        if (p.n_tiles * pl->n_rot > 65535) return PixPlan(COREG_EINVAL, "pixels: more than 65535 rotation planes x tiles");
        if (p.n_tiles * p.n_lag > (1ll << 28)) return PixPlan(COREG_EINVAL, "pixels: too many tiles x lags");
        tl.n_tiles = (int)p.n_tiles;
        tl.n_rot = pl->n_rot;
    }
    p.n_out = p.n_tiles * p.n_lag;
    const auto ex_dx = std::minmax_element(pl->lag_dx, pl->lag_dx + pl->n_dx);
    const auto ex_dy = std::minmax_element(pl->lag_dy, pl->lag_dy + pl->n_dy);
    p.min_dx = *ex_dx.first, p.max_dx = *ex_dx.second;
    p.min_dy = *ex_dy.first, p.max_dy = *ex_dy.second;
    // alignment_pixels.py:150-156, for every lag before any GPU work
    if ((long long)pl->l0 + p.min_dy < 0 || (long long)pl->l0 + p.max_dy + hh > pl->sub_ny || (long long)pl->l1 + p.min_dx < 0 ||
        (long long)pl->l1 + p.max_dx + w > pl->sub_nx)
        return PixPlan(COREG_EINVAL, "too large shift : outside FSI");
    for (int k = 0; k < pl->n_rot; ++k)
        if (!std::isfinite(pl->lag_drot[k])) return PixPlan(COREG_EINVAL, "pixels: a rotation lag is not finite");
    p.bW = w + (p.max_dx - p.min_dx);
    p.bH = hh + (p.max_dy - p.min_dy);
    if (pixels_too_many(p.bW, p.bH) || pixels_too_many((long long)w * hh, pl->n_rot))
        return PixPlan(COREG_EINVAL, "pixels: work space too large");

    p.groups = pixels_groups(pl->lag_dx, pl->n_dx);
    const int band_w = p.tiled ? p.tl.tw : w, band_h = p.tiled ? p.tl.th : hh;
    p.cw = std::min(band_w, kPixTile);
    p.bh = std::max(1, std::min(std::min(kPixBandRows, kPixTile / p.cw), band_h));
    assert(pixels_band_fits(p.cw, p.bh));
    p.grid[0] = (unsigned)p.groups.size();
    p.grid[1] = (unsigned)pl->n_dy;
    p.grid[2] = (unsigned)(pl->n_rot * p.n_tiles);
    p.fin_grid[0] = (unsigned)((p.n_lag + kPixThreads - 1) / kPixThreads);
    p.fin_grid[1] = (unsigned)p.n_tiles;
    p.off_dx = p.groups.size() * sizeof(PixGroup);
    p.off_dy = p.off_dx + (size_t)pl->n_dx * sizeof(int);
    p.off_a = p.off_b = p.bytes = p.off_dy + (size_t)pl->n_dy * sizeof(int);
    if (p.mi || p.lct) {
        p.n_a = p.mi ? have.n_edges_small : p.tl.th;
        p.n_b = p.mi ? have.n_edges_large : p.tl.tw;
        p.off_a = (p.bytes + 7) / 8 * 8;
        p.off_b = p.off_a + (size_t)p.n_a * sizeof(double);
        p.bytes = p.off_b + (size_t)p.n_b * sizeof(double);
    }
    return p;
}

// The blob of a plan, p.bytes of them: a, b are the edge lists (small, large) or the weight tables (wy, wx); unread without
inline void pixels_plan_write(const PixPlan& p, const coreg_pixels_plan* pl, const double* a, const double* b, unsigned char* blob) {
    std::memcpy(blob, p.groups.data(), p.off_dx);
    std::memcpy(blob + p.off_dx, pl->lag_dx, (size_t)pl->n_dx * sizeof(int));
    std::memcpy(blob + p.off_dy, pl->lag_dy, (size_t)pl->n_dy * sizeof(int));
    if (p.n_a) std::memcpy(blob + p.off_a, a, (size_t)p.n_a * sizeof(double));
    if (p.n_b) std::memcpy(blob + p.off_b, b, (size_t)p.n_b * sizeof(double));
}

// the section at `off` of a blob at `base` (host or device memory)
template <class T>
inline const T* pixels_plan_at(const void* base, size_t off) {
    return (const T*)((const unsigned char*)base + off);
}

}  // namespace coreg
