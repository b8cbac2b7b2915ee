// The lag planner and the slot layout (csrc/lag_plan.hpp) on the host, under sanitizers: for a list of lag planes --
// among them the headline's 60 x 60 and a slice of it that begins and ends in mid-row --
//   * every requested lag index occurs exactly once among the slots, nothing else does;
//   * the padding of a batch is the tail of its last live lag-wave and the whole lag-waves after it;
//   * no patch holds more than 256 lags, and the patches tile the plane;
//   * the live lag-waves do not exceed those of the single-rectangle plan of before, restated here on its own
//     (patch search, t % sw / t / sw slot layout, a lag-wave is live when one of its 64 slots holds a lag);
//   * 60 x 60 comes out at 57 live lag-waves (3600 / 64 = 56.25), and under the headline's geometry every patch's window
//     estimate fits the compiled pitch 121, which is also the pitch chosen for the launch;
//   * with `patch_w` set the plan is the single rectangle of before, batch for batch.
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <chrono>
#include <cstdio>
#include <set>

#include "../../euispice_coreg_amd/csrc/lag_plan.hpp"

using namespace lag_plan;

namespace {
constexpr int kTilePts = 1024;
constexpr long long kLdsElems = 159 * 1024 / 8;

int n_bad = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++n_bad;                       \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");             \
        }                                  \
    } while (0)

// ---- the plan of before, restated: one patch shape for the whole plane ----------------------------------------------
struct OldPlan {
    int tile_w, sw, sh;
};
OldPlan old_plan(const Geometry& g, int m1, int n2, long long lds, int patch_w) {
    OldPlan best = {32, 16, 16}, fb = best;
    double best_cost = 1e300, fb_win = 1e300;
    const int sw_hi = patch_w > 0 ? std::min(patch_w, 256) : 256;
    for (int tw = 4; tw <= 256; tw *= 2) {
        const int th = kTilePts / tw;
        const double tex = tw * std::fabs(g.dx_di) + th * std::fabs(g.dx_dj);
        const double tey = tw * std::fabs(g.dy_di) + th * std::fabs(g.dy_dj);
        for (int sw = 1; sw <= std::min(m1, sw_hi); ++sw) {
            int sh = std::min(n2, 256 / sw);
            if (sh < 1) break;
            const int cols = (m1 + sw - 1) / sw, rows = (n2 + sh - 1) / sh;
            sh = (n2 + rows - 1) / rows;
            const int sw2 = (m1 + cols - 1) / cols;
            const double ex = tex + sw2 * std::fabs(g.ax) + sh * std::fabs(g.bx) + 6.0;
            const double ey = tey + sw2 * std::fabs(g.ay) + sh * std::fabs(g.by) + 6.0;
            const double win = (ex + 1.0) * ey;
            if (win < fb_win) {
                fb_win = win;
                fb = {tw, sw2, sh};
            }
            if (win > 0.94 * (double)lds) continue;
            const double cost = (double)cols * rows * (1.0 + 0.08 * win / (double)lds);
            if (cost < best_cost) {
                best_cost = cost;
                best = {tw, sw2, sh};
            }
        }
    }
    return best_cost < 1e300 ? best : fb;
}
// its batches: the set of lag indices of each, and its live lag-waves under the slot layout of before
struct OldSlots {
    std::vector<std::set<long long>> batches;
    int live_waves = 0;
};
OldSlots old_slots(const LagDims& d, long long c, long long begin, long long end, int sw, int sh) {
    OldSlots o;
    const long long row = (long long)d.n2 * d.nc;
    const int i1_lo = (int)(begin / row), i1_hi = (int)((end - 1) / row);
    const int m1 = i1_hi - i1_lo + 1;
    for (int p1 = 0; p1 * sw < m1; ++p1)
        for (int p2 = 0; p2 * sh < d.n2; ++p2) {
            std::set<long long> lags;
            bool wave_live[4] = {false, false, false, false};
            for (int t = 0; t < 256; ++t) {
                const int lx = t % sw, ly = t / sw;
                if (ly >= sh) continue;
                const int i1 = i1_lo + p1 * sw + lx, i2 = p2 * sh + ly;
                if (i1 > i1_hi || i2 > d.n2 - 1) continue;
                const long long idx = ((long long)i1 * d.n2 + i2) * d.nc + c;
                if (idx < begin || idx >= end) continue;
                lags.insert(idx);
                wave_live[t / 64] = true;
            }
            if (lags.empty()) continue;
            o.batches.push_back(lags);
            for (bool w : wave_live) o.live_waves += w;
        }
    return o;
}

struct Case {
    const char* name;
    int n1, n2;
    long long begin, end;  // raveled slice; end < 0: the whole plane
    Geometry g;
};

Geometry headline_geometry() {
    // the benchmark's headline sweep (Carrington 2048^2 grid, 1" lags, 16 x 64 tiles): pixels per grid step / lag step
    Geometry g;
    g.dx_di = 4.440;
    g.dy_di = -0.233;
    g.dx_dj = 0.093;
    g.dy_dj = 1.774;
    g.ax = 2.030;
    g.ay = 0.106;
    g.bx = 0.106;
    g.by = 2.030;
    return g;
}

void run_case(const Case& cs, int* waves_out) {
    LagDims d = {cs.n1, cs.n2, 1, 1, 1, 1, 0};
    const long long begin = cs.begin, end = cs.end < 0 ? d.total() : cs.end;
    const long long row = (long long)d.n2 * d.nc;
    const int m1 = (int)((end - 1) / row) - (int)(begin / row) + 1;
    const Plan plan = plan_patches(cs.g, m1, cs.n2, kLdsElems, PlanOptions(), kTilePts);

    // the patches tile the m1 x n2 plane, none above 256 lags; live waves as declared
    std::vector<int> cover((size_t)m1 * cs.n2, 0);
    int waves = 0;
    for (const Rect& q : plan.rects) {
        CHECK(q.w >= 1 && q.h >= 1 && q.w * q.h <= kSlots, "%s: patch %d x %d", cs.name, q.w, q.h);
        CHECK(q.x0 >= 0 && q.y0 >= 0 && q.x0 + q.w <= m1 && q.y0 + q.h <= cs.n2, "%s: patch outside the plane", cs.name);
        if (q.x0 < 0 || q.y0 < 0 || q.x0 + q.w > m1 || q.y0 + q.h > cs.n2) continue;
        for (int x = 0; x < q.w; ++x)
            for (int y = 0; y < q.h; ++y) cover[(size_t)(q.x0 + x) * cs.n2 + q.y0 + y]++;
        waves += rect_waves(q.w, q.h);
    }
    for (int v : cover)
        if (v != 1) {
            CHECK(false, "%s: a lag of the plane is covered %d times", cs.name, v);
            break;
        }
    CHECK(waves == plan.live_waves, "%s: live_waves %d, patches say %d", cs.name, plan.live_waves, waves);

    SlotList s;
    build_slots(d, 0, begin, end, plan.rects, &s);
    CHECK(s.i1.size() == (size_t)s.n_batches * kSlots && s.i2.size() == s.i1.size() && s.outidx.size() == s.i1.size(),
          "%s: n_slots is not n_batches * 256", cs.name);
    std::vector<int> seen((size_t)(end - begin), 0);
    int live_waves = 0;
    for (int b = 0; b < s.n_batches; ++b) {
        int live = 0;
        bool padded = false;
        for (int t = 0; t < kSlots; ++t) {
            const size_t at = (size_t)b * kSlots + t;
            const long long idx = s.outidx[at];
            CHECK(s.i1[at] >= 0 && s.i1[at] < cs.n1 && s.i2[at] >= 0 && s.i2[at] < cs.n2, "%s: slot lag outside the axes", cs.name);
            if (idx < 0) {
                padded = true;
                continue;
            }
            CHECK(!padded, "%s: batch %d has a lag after padding (slot %d)", cs.name, b, t);
            CHECK(idx >= begin && idx < end, "%s: lag index %lld outside the slice", cs.name, idx);
            if (idx >= begin && idx < end) seen[(size_t)(idx - begin)]++;
            CHECK(idx == ((long long)s.i1[at] * d.n2 + s.i2[at]) * d.nc, "%s: index and (i1, i2) disagree", cs.name);
            ++live;
        }
        CHECK(live >= 1, "%s: batch %d is empty", cs.name, b);
        live_waves += (live + 63) / 64;  // (lags first, then padding: the live waves are the first ceil(live / 64))
    }
    for (size_t k = 0; k < seen.size(); ++k)
        if (seen[k] != 1) {
            CHECK(false, "%s: lag %lld occurs %d times", cs.name, begin + (long long)k, seen[k]);
            break;
        }
    CHECK(live_waves == s.live_waves, "%s: SlotList.live_waves %d, slots say %d", cs.name, s.live_waves, live_waves);
    CHECK(live_waves <= plan.live_waves, "%s: more live waves in the slots than planned", cs.name);

    // against the plan of before
    const OldPlan op = old_plan(cs.g, m1, cs.n2, kLdsElems, 0);
    const OldSlots os = old_slots(d, 0, begin, end, op.sw, op.sh);
    CHECK(live_waves <= os.live_waves, "%s: %d live waves, the single rectangle %d x %d had %d", cs.name, live_waves, op.sw,
          op.sh, os.live_waves);
    std::printf("%-22s %3d x %3d lags: tile %3d, %3d batches, %3d live waves (single rectangle %2d x %2d: %3zu batches, %3d)\n",
                cs.name, cs.n1, cs.n2, plan.tile_w, s.n_batches, live_waves, op.sw, op.sh, os.batches.size(), os.live_waves);
    if (waves_out) *waves_out = live_waves;

    // patch_w set: the batches of before, lag for lag
    for (int pw : {256, 7}) {
        PlanOptions o;
        o.patch_w = pw;
        const Plan forced = plan_patches(cs.g, m1, cs.n2, kLdsElems, o, kTilePts);
        const OldPlan fo = old_plan(cs.g, m1, cs.n2, kLdsElems, pw);
        const OldSlots want = old_slots(d, 0, begin, end, fo.sw, fo.sh);
        SlotList got;
        build_slots(d, 0, begin, end, forced.rects, &got);
        CHECK(forced.tile_w == fo.tile_w, "%s patch_w %d: tile %d, before %d", cs.name, pw, forced.tile_w, fo.tile_w);
        CHECK((size_t)got.n_batches == want.batches.size(), "%s patch_w %d: %d batches, before %zu", cs.name, pw, got.n_batches,
              want.batches.size());
        for (int b = 0; b < got.n_batches && (size_t)b < want.batches.size(); ++b) {
            std::set<long long> lags;
            for (int t = 0; t < kSlots; ++t)
                if (got.outidx[(size_t)b * kSlots + t] >= 0) lags.insert(got.outidx[(size_t)b * kSlots + t]);
            CHECK(lags == want.batches[(size_t)b], "%s patch_w %d: batch %d holds other lags than before", cs.name, pw, b);
        }
    }
}
}  // namespace

int main() {
    const Geometry hg = headline_geometry();
    Geometry unit;  // one pixel per grid step, no lag motion: every window fits
    const Case cases[] = {
        {"60x60 headline", 60, 60, 0, -1, hg},       {"61x61", 61, 61, 0, -1, hg},
        {"121x121", 121, 121, 0, -1, hg},           {"41x41", 41, 41, 0, -1, hg},
        {"30x30", 30, 30, 0, -1, hg},               {"1x300", 1, 300, 0, -1, unit},
        {"300x1", 300, 1, 0, -1, unit},             {"7x37", 7, 37, 0, -1, hg},
        {"16x12", 16, 12, 0, -1, hg},               {"8x8", 8, 8, 0, -1, hg},
        {"1x1", 1, 1, 0, -1, hg},                   {"60x60 mid-row slice", 60, 60, 60 * 13 + 17, 60 * 47 + 5, hg},
        {"60x60 unit geometry", 60, 60, 0, -1, unit}, {"60x60 slice in a row", 60, 60, 60 * 20 + 3, 60 * 20 + 41, unit},
    };
    int waves_headline = -1;
    for (const Case& cs : cases) run_case(cs, &cs == &cases[0] ? &waves_headline : nullptr);
    CHECK(waves_headline == 57, "60 x 60: %d live waves, not 57", waves_headline);
    {
        int w = -1;
        run_case(cases[12], &w);
        CHECK(w == 57, "60 x 60, unit geometry: %d live waves, not 57", w);
    }
    // the headline's windows and its pitch
    {
        const Plan plan = plan_patches(hg, 60, 60, kLdsElems, PlanOptions(), kTilePts);
        CHECK(plan.tile_w == 16, "headline: tile width %d, not 16", plan.tile_w);
        const int th = kTilePts / plan.tile_w;
        const double tex = plan.tile_w * std::fabs(hg.dx_di) + th * std::fabs(hg.dx_dj);
        const double tey = plan.tile_w * std::fabs(hg.dy_di) + th * std::fabs(hg.dy_dj);
        for (const Rect& q : plan.rects) {
            const double ww = tex + q.w * std::fabs(hg.ax) + q.h * std::fabs(hg.bx) + 7.0;
            const double wh = tey + q.w * std::fabs(hg.ay) + q.h * std::fabs(hg.by) + 6.0;
            CHECK(ww + 2.0 <= 121.0 && 121.0 * wh <= 0.985 * (double)kLdsElems && ww * wh <= 0.94 * (double)kLdsElems,
                  "headline: patch %d x %d has a window estimate of %.1f x %.1f, beyond pitch 121", q.w, q.h, ww, wh);
        }
        CHECK(pitch_for(plan, kLdsElems, 2) == 121, "headline: pitch %d, not 121", pitch_for(plan, kLdsElems, 2));
        std::printf("headline patches:");
        for (const Rect& q : plan.rects) std::printf(" %dx%d", q.w, q.h);
        std::printf("; window estimate %.1f x %.1f\n", plan.win_w, plan.win_h);
        const auto t0 = std::chrono::steady_clock::now();
        int sink = 0;
        for (int k = 0; k < 200; ++k) sink += plan_patches(hg, 60, 60, kLdsElems, PlanOptions(), kTilePts).live_waves;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 200.0;
        std::printf("planning the headline: %.1f us per call (%d)\n", us, sink);
    }
    // a patch of more than 256 lags is no plan's; handed to build_slots all the same, it loses no lag
    {
        LagDims d = {20, 30, 1, 1, 1, 1, 0};
        const std::vector<Rect> one = {{0, 0, 20, 30}};
        SlotList s;
        build_slots(d, 0, 0, d.total(), one, &s);
        std::set<long long> lags;
        for (long long idx : s.outidx)
            if (idx >= 0) {
                CHECK(lags.insert(idx).second, "oversize patch: lag %lld twice", idx);
            }
        CHECK(s.n_batches == 3 && s.outidx.size() == 3u * kSlots && lags.size() == 600u && s.live_waves == 10,
              "oversize patch: %d batches, %zu slots, %zu lags, %d live waves", s.n_batches, s.outidx.size(), lags.size(),
              s.live_waves);
    }
    // the planes of tests/test_gpu_lag_packing.py (small images: every window fits): between them their batches have one,
    // two, three and four live lag-waves, a last wave that is not full among them
    {
        const int planes[][2] = {{8, 8}, {9, 15}, {16, 12}, {20, 20}, {33, 17}, {8, 16}};
        bool kind[5] = {false, false, false, false, false}, ragged = false;
        for (const auto& pl : planes) {
            const Plan plan = plan_patches(unit, pl[0], pl[1], kLdsElems, PlanOptions(), kTilePts);
            std::printf("%d x %d:", pl[0], pl[1]);
            for (const Rect& q : plan.rects) {
                kind[rect_waves(q.w, q.h)] = true;
                ragged = ragged || (q.w * q.h) % kWaveLags != 0;
                std::printf(" %dx%d", q.w, q.h);
            }
            std::printf("\n");
        }
        CHECK(kind[1] && kind[2] && kind[3] && kind[4] && ragged, "GPU test planes: live-wave kinds %d %d %d %d, ragged %d",
              (int)kind[1], (int)kind[2], (int)kind[3], (int)kind[4], (int)ragged);
    }
    if (n_bad) return 1;
    std::printf("ok: %zu lag planes\n", sizeof(cases) / sizeof(cases[0]));
    return 0;
}
