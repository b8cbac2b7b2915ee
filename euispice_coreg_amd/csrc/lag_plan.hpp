// How the (CRVAL1 x CRVAL2) lag plane of a sweep is cut into batches of <= 256 lags (one k_sweep workgroup each) and how
// the lags of a batch are laid over its 256 slots.  Plain C++ with no HIP dependency: included by sweep_plan.hpp (part
// of libcoreg_hip.so's one translation unit), and tests/native/lag_plan_rules.cpp walks it on the host under sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace lag_plan {
constexpr int kSlots = 256;    // lag slots of a batch (kernels_common.hpp: kBlock), four lag-waves of 64
constexpr int kWaveLags = 64;

struct LagDims {
    int n1, n2, n3, n4, n5;
    long long nc;  // (cdelt1, cdelt2, crota) combinations this sweep covers: n3*n4*n5, or the "combo_begin/_end" range
    long long c0;  // first of them in the lag set's inner C-order index ((i3 * n4 + i4) * n5 + i5)
    long long total() const { return (long long)n1 * n2 * nc; }
    void inner(long long c, int* i3, int* i4, int* i5) const {  // c in [0, nc)
        const long long g = c + c0;
        *i5 = (int)(g % n5);
        *i4 = (int)((g / n5) % n4);
        *i3 = (int)(g / ((long long)n5 * n4));
    }
};

// Local pixel-space geometry of a sweep (host estimates; they steer the plan, never the results):
// small-image pixels per grid step (d?_di, d?_dj) and per CRVAL1 / CRVAL2 lag step (a?, b?).
struct Geometry {
    double dx_di = 1, dx_dj = 0, dy_di = 0, dy_dj = 1;
    double ax = 0, ay = 0, bx = 0, by = 0;
};

// One lag patch = one batch: CRVAL1 lags [x0, x0 + w) of the slice's rows x CRVAL2 lags [y0, y0 + h), w * h <= kSlots.
struct Rect {
    int x0, y0, w, h;
};
inline int rect_waves(int w, int h) { return (w * h + kWaveLags - 1) / kWaveLags; }

struct Plan {
    int tile_w = 32;          // grid tile = tile_w x (tile_pts / tile_w) points
    std::vector<Rect> rects;  // guillotine cut of the lag plane: column strips, each cut into row blocks; strip-major
    int live_waves = 0;       // sum over the patches of ceil(w * h / 64): the lag-waves that hold a lag
    double window = 0;        // largest estimated LDS window of a patch (elements)
    double win_w = 0, win_h = 0;  // the largest estimated width / height of a patch's window in pixels
};

struct PlanOptions {
    int tile_w = 0;   // > 0: this tile width only
    int patch_w = 0;  // > 0: ONE patch shape tiles the plane, at most this wide (the plan of before the patches were packed)
};

namespace detail {
struct TileExtent {
    double tex, tey;
};
inline TileExtent tile_extent(const Geometry& g, int tw, int th) {
    return {tw * std::fabs(g.dx_di) + th * std::fabs(g.dx_dj), tw * std::fabs(g.dy_di) + th * std::fabs(g.dy_dj)};
}
// estimated window of tile (+) patch: width (apron and slack included), height, elements
inline void window_of(const Geometry& g, const TileExtent& t, int w, int h, double* ww, double* wh, double* win) {
    const double ex = t.tex + w * std::fabs(g.ax) + h * std::fabs(g.bx) + 6.0;
    const double ey = t.tey + w * std::fabs(g.ay) + h * std::fabs(g.by) + 6.0;
    *ww = ex + 1.0;
    *wh = ey;
    *win = (ex + 1.0) * ey;
}
inline bool fits(double win, long long lds_elems) { return win <= 0.94 * (double)lds_elems; }

// (live waves, batches, widest strip) of a partial cut, compared in that order
struct Cost {
    int waves = 0, batches = 0, wmax = 0;
    bool operator<(const Cost& o) const {
        if (waves != o.waves) return waves < o.waves;
        if (batches != o.batches) return batches < o.batches;
        return wmax < o.wmax;
    }
};
constexpr int kNever = 1 << 28;

// A strip `w` lags wide over n rows, blocks at most hcap rows high: the cut with the fewest live waves, then the
// fewest blocks.  Some best cut has every block but one as high as its wave count allows (a block of k waves that is
// lower can grow into its neighbour at no cost), so the blocks are the up to four heights floor(64 k / w) and one rest.
// Blocks of equal waves are then evened out (12 lags wide over 60 rows: 20 + 20 + 20, not 21 + 21 + 18): the launch's
// LDS pitch is sized for the highest window.
struct StripCutter {
    std::vector<long long> f;  // (waves << 32) + blocks of the best cut of the first r rows into full-height blocks
    std::vector<int> from;
    Cost cut(int w, int n, int hcap, std::vector<int>* heights) {
        constexpr long long kInf = std::numeric_limits<long long>::max() / 2;
        int hk[4], nk = 0;
        long long ck[4];
        for (int k = 1; k <= kSlots / kWaveLags; ++k) {
            const int h = std::min(hcap, k * kWaveLags / w);
            if (h < 1 || (nk > 0 && h == hk[nk - 1])) continue;
            hk[nk] = h;
            ck[nk] = ((long long)rect_waves(w, h) << 32) + 1;
            ++nk;
        }
        f.resize((size_t)n + 1);
        from.resize((size_t)n + 1);
        f[0] = 0;
        for (int r = 1; r <= n; ++r) {
            long long best = kInf;
            int bk = -1;
            for (int k = 0; k < nk; ++k) {
                if (hk[k] > r) break;
                const long long c = f[(size_t)(r - hk[k])] + ck[k];
                if (c < best) {
                    best = c;
                    bk = k;
                }
            }
            f[(size_t)r] = best;
            from[(size_t)r] = bk;
        }
        long long best = kInf;
        int best_r = -1;
        for (int rest = 0; rest <= std::min(hcap, n); ++rest) {
            long long c = f[(size_t)(n - rest)];
            if (c >= kInf) continue;
            if (rest > 0) c += ((long long)rect_waves(w, rest) << 32) + 1;
            if (c < best) {
                best = c;
                best_r = n - rest;
            }
        }
        Cost out;
        out.waves = kNever;
        if (best_r < 0) return out;
        out.waves = (int)(best >> 32);
        out.batches = (int)(best & 0xffffffffll);
        out.wmax = w;
        if (heights) {
            heights->clear();
            for (int r = best_r; r > 0; r -= hk[from[(size_t)r]]) heights->push_back(hk[from[(size_t)r]]);
            if (n - best_r > 0) heights->push_back(n - best_r);
            std::sort(heights->begin(), heights->end(), [](int a, int b) { return a > b; });  // (the low block last, as before)
            // even out: move a row from the highest block to the lowest while no block gains a wave
            for (;;) {
                int& hi = heights->front();
                int& lo = heights->back();
                if (hi - lo < 2 || rect_waves(w, hi - 1) + rect_waves(w, lo + 1) > rect_waves(w, hi) + rect_waves(w, lo)) break;
                --hi;
                ++lo;
                std::sort(heights->begin(), heights->end(), [](int a, int b) { return a > b; });
            }
        }
        return out;
    }
};

// the plan of before: ONE patch shape (sw x sh, cut short at the plane's far edges) tiles the plane -- fewest batches
// among the tile shapes / patch shapes whose window fits, ties -> smaller window; nothing fits: the smallest window
inline Plan single_patch_plan(const Geometry& g, int m1, int n2, long long lds_elems, const PlanOptions& o, int tile_pts) {
    struct Pick {
        int tile_w = 32, sw = 16, sh = 16;
    } best, fallback;
    double best_cost = std::numeric_limits<double>::max(), fb_win = std::numeric_limits<double>::max();
    const int sw_hi = o.patch_w > 0 ? std::min(o.patch_w, kSlots) : kSlots;
    for (int tw = 4; tw <= 256; tw *= 2) {
        if (o.tile_w > 0 && tw != o.tile_w) continue;
        const int th = tile_pts / tw;
        if (th < 1) continue;
        const TileExtent te = tile_extent(g, tw, th);
        for (int sw = 1; sw <= std::min(m1, sw_hi); ++sw) {
            int sh = std::min(n2, kSlots / sw);
            if (sh < 1) break;
            const int cols = (m1 + sw - 1) / sw, rows = (n2 + sh - 1) / sh;
            sh = (n2 + rows - 1) / rows;             // smallest sh with the same batch count
            const int sw2 = (m1 + cols - 1) / cols;  // likewise for sw
            double ww, wh, win;
            window_of(g, te, sw2, sh, &ww, &wh, &win);
            if (win < fb_win) {
                fb_win = win;
                fallback.tile_w = tw;
                fallback.sw = sw2;
                fallback.sh = sh;
            }
            if (!fits(win, lds_elems)) continue;
            const double cost = (double)cols * rows * (1.0 + 0.08 * win / (double)lds_elems);
            if (cost < best_cost) {
                best_cost = cost;
                best.tile_w = tw;
                best.sw = sw2;
                best.sh = sh;
            }
        }
    }
    const Pick& r = best_cost < std::numeric_limits<double>::max() ? best : fallback;
    Plan p;
    p.tile_w = r.tile_w;
    for (int x0 = 0; x0 < m1; x0 += r.sw)
        for (int y0 = 0; y0 < n2; y0 += r.sh) {
            const Rect q = {x0, y0, std::min(r.sw, m1 - x0), std::min(r.sh, n2 - y0)};
            p.rects.push_back(q);
            p.live_waves += rect_waves(q.w, q.h);
        }
    window_of(g, tile_extent(g, r.tile_w, tile_pts / r.tile_w), r.sw, r.sh, &p.win_w, &p.win_h, &p.window);
    return p;
}
}  // namespace detail

// Tile shape and lag patches chosen together.  m1 x n2 = lag plane (m1 CRVAL1 rows of the slice).  The plane is cut
// guillotine-fashion: column strips of CRVAL1 lags, each strip into blocks of CRVAL2 lags, every block a patch of
// <= 256 lags whose LDS window (tile extent (+) patch extent, in pixels) fits.  Chosen: the fewest live lag-waves,
// sum of ceil(w h / 64) -- k_sweep gives a SIMD one wave per live lag-wave of a batch, so that sum is the work -- then
// the fewest batches weighted by the window as before.  When no patch fits, or with `patch_w` set: single_patch_plan.
inline Plan plan_patches(const Geometry& g, int m1, int n2, long long lds_elems, const PlanOptions& o, int tile_pts) {
    using namespace detail;
    if (o.patch_w > 0 || m1 < 1 || n2 < 1) return single_patch_plan(g, m1, n2, lds_elems, o, tile_pts);
    Plan best;
    double best_cost = std::numeric_limits<double>::max();
    int best_waves = kNever;
    const int wmax = std::min(m1, kSlots);
    std::vector<Cost> strip((size_t)wmax + 1), col((size_t)m1 + 1);
    std::vector<int> hcap((size_t)wmax + 1), memo_hcap((size_t)wmax + 1, -1), pick((size_t)m1 + 1);
    std::vector<Cost> memo((size_t)wmax + 1);
    std::vector<int> heights;
    StripCutter cutter;
    for (int tw = 4; tw <= 256; tw *= 2) {
        if (o.tile_w > 0 && tw != o.tile_w) continue;
        const int th = tile_pts / tw;
        if (th < 1) continue;
        const TileExtent te = tile_extent(g, tw, th);
        // every strip width: the highest block whose window fits, and the strip's best cut
        int w_fit = 0, h_prev = n2;
        for (int w = 1; w <= wmax; ++w) {
            int h = std::min(h_prev, kSlots / w);  // (the cap cannot grow with the width)
            double ww, wh, win;
            for (; h >= 1; --h) {
                window_of(g, te, w, h, &ww, &wh, &win);
                if (fits(win, lds_elems)) break;
            }
            if (h < 1) break;  // (wider strips have larger windows still)
            hcap[(size_t)w] = h_prev = h;
            if (memo_hcap[(size_t)w] != h) {  // (the cut depends on the tile shape only through the cap)
                memo[(size_t)w] = cutter.cut(w, n2, h, nullptr);
                memo_hcap[(size_t)w] = h;
            }
            strip[(size_t)w] = memo[(size_t)w];
            w_fit = w;
        }
        if (w_fit < 1) continue;
        // the column strips
        col[0] = Cost();
        for (int c = 1; c <= m1; ++c) {
            col[(size_t)c].waves = kNever;
            for (int w = 1; w <= std::min(c, w_fit); ++w) {
                const Cost& a = col[(size_t)(c - w)];
                if (a.waves >= kNever) continue;
                Cost s = {a.waves + strip[(size_t)w].waves, a.batches + strip[(size_t)w].batches, std::max(a.wmax, w)};
                if (s < col[(size_t)c]) {
                    col[(size_t)c] = s;
                    pick[(size_t)c] = w;
                }
            }
        }
        const Cost& total = col[(size_t)m1];
        if (total.waves >= kNever || total.waves > best_waves) continue;
        // its patches, its largest window, and the cost of before for ties
        Plan p;
        p.tile_w = tw;
        p.live_waves = total.waves;
        std::vector<int> widths;
        for (int c = m1; c > 0; c -= pick[(size_t)c]) widths.push_back(pick[(size_t)c]);
        std::sort(widths.begin(), widths.end(), [](int a, int b) { return a > b; });  // (the narrow strip last, as before)
        int x0 = 0;
        for (int w : widths) {
            cutter.cut(w, n2, hcap[(size_t)w], &heights);
            int y0 = 0;
            for (int h : heights) {
                p.rects.push_back({x0, y0, w, h});
                double ww, wh, win;
                window_of(g, te, w, h, &ww, &wh, &win);
                p.win_w = std::max(p.win_w, ww);
                p.win_h = std::max(p.win_h, wh);
                p.window = std::max(p.window, win);
                y0 += h;
            }
            x0 += w;
        }
        const double cost = (double)total.batches * (1.0 + 0.08 * p.window / (double)lds_elems);
        if (total.waves < best_waves || cost < best_cost) {
            best_waves = total.waves;
            best_cost = cost;
            best = p;
        }
    }
    if (best_waves >= kNever) return single_patch_plan(g, m1, n2, lds_elems, o, tile_pts);
    return best;
}

struct SlotList {
    std::vector<int> i1, i2;        // lag indices supplying the lane parameters (a live lag's, or the patch's first for padding)
    std::vector<long long> outidx;  // raveled C-order lag index or -1
    int n_batches = 0;
    int live_waves = 0;             // lag-waves (64 slots) that hold at least one lag
};

// Slots for combo c (= (i3*n4 + i4)*n5 + i5) restricted to the raveled slice [begin, end): one batch of kSlots slots per
// patch of the plan that holds a lag of the slice.  The lags of a patch fill the batch's first slots in the patch's
// row-major order (CRVAL1 fastest): the padding (outidx -1) is the tail of the last live lag-wave and the whole lag-waves
// after it, which k_sweep's waves skip.  (No plan has a patch of more than kSlots lags; one handed in all the same is
// spread over as many batches as it needs, so no lag is ever left out.)
inline void build_slots(const LagDims& d, long long c, long long begin, long long end, const std::vector<Rect>& rects,
                        SlotList* s) {
    s->i1.clear();
    s->i2.clear();
    s->outidx.clear();
    s->n_batches = 0;
    s->live_waves = 0;
    if (end <= begin) return;
    s->i1.reserve(rects.size() * kSlots);
    s->i2.reserve(rects.size() * kSlots);
    s->outidx.reserve(rects.size() * kSlots);
    const long long row = (long long)d.n2 * d.nc;
    const int i1_lo = (int)(begin / row);
    const int i1_hi = (int)((end - 1) / row);
    // pads the batch begun at slot `at` to kSlots with its first lag's indices and counts it
    auto close_batch = [s](size_t at) {
        const size_t live = s->i1.size() - at;
        const int p1 = s->i1[at], p2 = s->i2[at];
        s->i1.resize(at + kSlots, p1);
        s->i2.resize(at + kSlots, p2);
        s->outidx.resize(at + kSlots, -1);
        s->n_batches++;
        s->live_waves += (int)((live + kWaveLags - 1) / kWaveLags);
    };
    for (const Rect& q : rects) {
        size_t at = s->i1.size();
        for (int ly = 0; ly < q.h; ++ly)
            for (int lx = 0; lx < q.w; ++lx) {
                const int i1 = i1_lo + q.x0 + lx, i2 = q.y0 + ly;
                if (i1 > i1_hi || i2 > d.n2 - 1) continue;
                const long long idx = ((long long)i1 * d.n2 + i2) * d.nc + c;
                if (idx < begin || idx >= end) continue;
                if (s->i1.size() - at == (size_t)kSlots) {  // (the batch is full: the patch goes on in another)
                    close_batch(at);
                    at = s->i1.size();
                }
                s->i1.push_back(i1);
                s->i2.push_back(i2);
                s->outidx.push_back(idx);
            }
        if (s->i1.size() > at) close_batch(at);  // (else: no lag of the slice in this patch)
    }
}

// Compile-time LDS window pitch for the order-2 / order-3 sweeps: the smallest instantiated pitch that holds the plan's
// widest window (width + slack) and, with its highest, stays within the LDS -- a launch has one pitch for all its
// patches.  All of them are 25 mod 32, the residue that spreads the ~2 px lag lattice best over the 32 bank pairs in the
// conflict simulation.  0 = pitch chosen per visit.
inline int pitch_for(const Plan& plan, long long lds_elems, int order) {
    static const int kPitches[] = {89, 121, 153, 185, 217};
    for (int p : kPitches)
        if ((double)p >= plan.win_w + (order > 2 ? 4.0 : 2.0) &&
            (double)p * (plan.win_h + (order > 2 ? 2.0 : 0.0)) <= 0.985 * (double)lds_elems)
            return p;
    return 0;
}
}  // namespace lag_plan
