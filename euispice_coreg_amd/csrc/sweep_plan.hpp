// The deciding half of the three header-shift sweeps (coreg_sweep_carrington; coreg_sweep_helioprojective, TAN and
// CAR): from a validated call, the headers and a read-only description of the handle (SweepEnv) to a SweepPlan -- the lane
// parameters and output indices of every slot, the launches with their cull boxes and uniforms, and the lag-points that
// wcslib's rounding noise decides.  Nothing here touches the device: abi_sweeps.hpp's run_sweep_plan turns a
// plan into uploads and launches.  Plain C++ with no HIP dependency (launch_uniforms.hpp is the part of the kernels'
// argument structs the plan speaks in); tests/native/sweep_plan_rules.cpp states its rules and runs them on the host,
// plain and under sanitizers.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "geometry.hpp"
#include "lag_plan.hpp"
#include "launch_uniforms.hpp"

namespace coreg {

// COREG_TRACE=1: host-side timestamps (microseconds since the first one) of the hand-over's stages on stderr
inline void trace(const char* what) {
    static const bool on = [] {
        const char* e = std::getenv("COREG_TRACE");
        return e && std::atoi(e) == 1;
    }();
    if (!on) return;
    static const auto t0 = std::chrono::steady_clock::now();
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[coreg %9.1f us] %s\n", us, what);
}

// ---- host fork/join ---------------------------------------------------------------------------------------------
// fn(lo, hi) over [0, n) in chunks of `grain` items (0: one even share per thread) dealt from a shared counter, on up to
// `max_threads` threads, this one included, and never more than there are chunks or cores.  Every caller's items are
// independent of one another, so the split never changes a result.  Work run here must not touch the handle's caches.
template <typename Fn>
void parallel_for(long long n, unsigned max_threads, long long grain, Fn fn) {
    if (n <= 0) return;
    const long long nt_max = std::max<long long>(1, std::min(max_threads, std::thread::hardware_concurrency()));
    if (grain <= 0) grain = (n + nt_max - 1) / nt_max;
    const long long nt = std::min(nt_max, (n + grain - 1) / grain);
    if (nt <= 1) {
        fn(0ll, n);
        return;
    }
    std::atomic<long long> next(0);
    auto worker = [&] {
        for (long long lo = next.fetch_add(grain); lo < n; lo = next.fetch_add(grain)) fn(lo, std::min(n, lo + grain));
    };
    std::vector<std::thread> th;
    for (long long t = 1; t < nt; ++t) th.emplace_back(worker);
    worker();
    for (auto& x : th) x.join();
}

// ---- lag batching (lag_plan.hpp: the planner and the slot layout) -----------------------------------------------------
using lag_plan::Geometry;
using lag_plan::LagDims;
using lag_plan::Plan;
using lag_plan::SlotList;
using lag_plan::build_slots;
static_assert(lag_plan::kSlots == kBlock && lag_plan::kWaveLags == 64, "lag_plan.hpp restates the kernels' constants");

// ---- what planning may read of the handle, and the state it may update ------------------------------------------------
// Zero-lag border decisions (geometry.hpp WcslibTan / WcslibCar): the grid pixels the reference's wcslib round trip drops
// and the tap-shift flags of every grid pixel, cached per header pair.  Owned by the handle.
struct WcslibCaches {
    std::map<std::vector<double>, std::vector<int>> border;          // at most 64 entries, cleared when full
    std::map<std::vector<double>, std::vector<unsigned char>> flags;  // at most 4
};
// the last lag plan and what it was made from (choose_plan): a session sweeps one lag set under one geometry many times,
// and planning the headline's 60 x 60 lags takes about 65 us on the host (tests/native/lag_plan_rules.cpp prints
// it), 2 % of its 3.2 ms step with one sweep in flight; keyed on every input of the planner, so it cannot go stale
struct PlanMemo {
    bool valid = false;
    Geometry g;
    int m1 = 0, n2 = 0;
    long long lds_elems = 0;
    lag_plan::PlanOptions o;
    Plan plan;
};
struct SweepEnv {
    int sW = 0, sH = 0, gW = 0, gH = 0;  // the image to align, the target grid
    bool border_fix = true, tap_fix = true, use_lds = true, h_series = true, tile_skip = true;
    long long lds_elems = 0;  // elements of the LDS window (read with use_lds)
    int tile_w = 0, patch_w = 0;
    long long shard_world = 1, n_groups = 0, pitch = -1;
    const CarrTables* tabs = nullptr;  // the Carrington host tables of this call's grid (plan_carrington)
    unsigned plan_threads = 0;         // threads of plan_tan's per-combination pass; 0: by the size of the lag set
    WcslibCaches* caches = nullptr;    // updated
    PlanMemo* memo = nullptr;          // updated
};

// Tile groups of a launch.  The compacted points are cut in n_groups EQUAL shares (k_tile_list), so n_groups * n_batches
// workgroups of equal work: 256 groups make every round of 256 CUs full; fewer when there are many lag batches.
inline int pick_groups(long long shard_world, long long opt_n_groups, int n_batches) {
    if (shard_world > 1) {
        // point sharding: every rank takes a multiple of 8 groups (the XCD-aware block mapping of k_sweep), as close
        // to one full round of 256 workgroups as the batch count allows
        const long long per_rank = 8 * std::max<long long>(1, std::llround(256.0 / (8.0 * n_batches)));
        return (int)std::min<long long>(per_rank * shard_world, 1000 / (8 * shard_world) * 8 * shard_world);
    }
    long long g = opt_n_groups > 0 ? opt_n_groups : (4096 + n_batches - 1) / n_batches;
    g = std::max<long long>(8, std::min<long long>(opt_n_groups > 0 ? 1000 : 256, ((g + 7) / 8) * 8));
    return (int)g;
}

// Compile-time LDS window pitch of a launch (lag_plan::pitch_for) under the "pitch" option.  0 = pitch chosen per visit.
inline int pick_pitch(long long opt_pitch, bool use_lds, const Plan& plan, long long lds_elems, int order = 2) {
    if (opt_pitch == 0 || !use_lds) return 0;
    if (opt_pitch > 0) {
        for (int p : {89, 121, 153, 185, 217})
            if (p == opt_pitch) return p;
        return 0;
    }
    return lag_plan::pitch_for(plan, lds_elems, order);
}

// Tile shape and lag patches of a sweep (lag_plan::plan_patches) under the handle's options.  m1 x n2 = lag plane.
inline Plan choose_plan(const SweepEnv& env, const Geometry& g, int m1, int n2, long long lds_elems) {
    lag_plan::PlanOptions o;
    o.tile_w = env.tile_w;
    o.patch_w = env.patch_w;
    PlanMemo& memo = *env.memo;
    const bool same = memo.valid && memo.m1 == m1 && memo.n2 == n2 && memo.lds_elems == lds_elems && memo.o.tile_w == o.tile_w &&
                      memo.o.patch_w == o.patch_w && std::memcmp(&memo.g, &g, sizeof(g)) == 0;
    if (!same) {
        memo.plan = lag_plan::plan_patches(g, m1, n2, lds_elems, o, kTilePts);
        memo.g = g;
        memo.m1 = m1;
        memo.n2 = n2;
        memo.lds_elems = lds_elems;
        memo.o = o;
        memo.valid = true;
    }
    const Plan& r = memo.plan;
    if (std::getenv("COREG_DEBUG_PLAN")) {
        std::string patches;
        for (size_t k = 0; k < r.rects.size(); ++k) {
            size_t n = 1;
            while (k + n < r.rects.size() && r.rects[k + n].w == r.rects[k].w && r.rects[k + n].h == r.rects[k].h) ++n;
            patches += (patches.empty() ? "" : " + ") + std::to_string(n) + " of " + std::to_string(r.rects[k].w) + " x " +
                       std::to_string(r.rects[k].h);
            k += n - 1;
        }
        std::fprintf(stderr, "[coreg plan] tile %d x %d, lag patches %s = %d live lag-waves, window estimate %.0f (%.1f x %.1f) of %lld elements; "
                     "geometry d/di (%.3f, %.3f) d/dj (%.3f, %.3f) lag1 (%.3f, %.3f) lag2 (%.3f, %.3f)\n", r.tile_w,
                     kTilePts / r.tile_w, patches.c_str(), r.live_waves, r.window, r.win_w, r.win_h, lds_elems, g.dx_di, g.dy_di,
                     g.dx_dj, g.dy_dj, g.ax, g.ay, g.bx, g.by);
    }
    return r;
}

// indices of the smallest, the most central and the largest value of a lag axis (any order, NaNs ignored)
inline void extreme_lags(const double* v, int n, int out[3]) {
    int lo = 0, hi = 0;
    for (int i = 1; i < n; ++i) {
        if (v[i] < v[lo] || v[lo] != v[lo]) lo = i;
        if (v[i] > v[hi] || v[hi] != v[hi]) hi = i;
    }
    const double mid = 0.5 * (v[lo] + v[hi]);
    int m = lo;
    for (int i = 0; i < n; ++i)
        if (std::fabs(v[i] - mid) < std::fabs(v[m] - mid)) m = i;
    out[0] = lo;
    out[1] = m;
    out[2] = hi;
}

// mean spacing of a lag axis over its value range (plan heuristics only; lists may come in any order)
inline double lag_step(const double* v, int n) {
    if (n < 2) return 0.0;
    double lo = v[0], hi = v[0];
    for (int i = 1; i < n; ++i) {
        lo = std::min(lo, v[i]);
        hi = std::max(hi, v[i]);
    }
    return (hi - lo) / (double)(n - 1);
}

// ---- the call ---------------------------------------------------------------------------------------------------------
// A sweep call between open_sweep and end_sweep: its lag set and slice, and where the results go.
struct SweepCall {
    const coreg_lags* lags = nullptr;
    LagDims d;
    int order = 0, method = 0, sem = 0;
    long long lag_begin = 0, lag_end = 0, n_out = 0;
    double* corr_out = nullptr;
    int out_on_device = 0;
    double* out_dev = nullptr;
    long long row() const { return (long long)d.n2 * d.nc; }  // lag indices per CRVAL1 value
    int i1_lo() const { return (int)(lag_begin / row()); }
    int i1_hi() const { return (int)((lag_end - 1) / row()); }
};

// Local geometry from the maps of the central CRVAL lag and of that lag plus one mean step on either axis, about the
// middle of the target grid.  at(v1, v2, u, v, &x, &y): target pixel (u, v) under the CRVAL lag (v1, v2); false: that
// lag has no map (any plan will do then, its lanes are NaN).
template <typename MapAt>
Geometry local_geometry(const coreg_wcs2d& target, const SweepCall& call, MapAt at) {
    const coreg_lags& l = *call.lags;
    int e1[3], e2[3];
    extreme_lags(l.crval1, call.d.n1, e1);
    extreme_lags(l.crval2, call.d.n2, e2);
    const double v1 = l.crval1[e1[1]], v2 = l.crval2[e2[1]];
    const double s1 = lag_step(l.crval1, call.d.n1), s2 = lag_step(l.crval2, call.d.n2);
    const double u = target.naxis1 * 0.5, v = target.naxis2 * 0.5;
    double x0, y0, xi, yi, xj, yj, xa, ya, xb, yb;
    Geometry g;
    if (!at(v1, v2, u, v, &x0, &y0) || !at(v1, v2, u + 1, v, &xi, &yi) || !at(v1, v2, u, v + 1, &xj, &yj) ||
        !at(v1 + s1, v2, u, v, &xa, &ya) || !at(v1, v2 + s2, u, v, &xb, &yb))
        return g;
    g.dx_di = xi - x0;
    g.dy_di = yi - y0;
    g.dx_dj = xj - x0;
    g.dy_dj = yj - y0;
    g.ax = xa - x0;
    g.ay = ya - y0;
    g.bx = xb - x0;
    g.by = yb - y0;
    return g;
}

// tile shape + lag patch for the CRVAL1 rows of the slice
inline Plan plan_lags(const SweepEnv& env, const Geometry& geo, const SweepCall& call) {
    return choose_plan(env, geo, call.i1_hi() - call.i1_lo() + 1, call.d.n2, env.use_lds ? env.lds_elems : (1LL << 40));
}

// Combination c of the sweep: its (CDELT, CROTA)-shifted header and its lag slots.  False: nothing of it to launch (no
// lag of the slice, or a lag that kills the reference's worker: NaN, already filled).  Pure: called from threads.
inline bool combo_slots(const SweepCall& call, const coreg_wcs2d& small, const Plan& plan, long long c, coreg_wcs2d* hc,
                        SlotList* slots) {
    const long long first = (call.lag_begin - c + call.d.nc - 1) / call.d.nc;  // smallest k with k*nc + c >= begin
    if (first * call.d.nc + c >= call.lag_end) return false;
    int i3, i4, i5;
    call.d.inner(c, &i3, &i4, &i5);
    if (shift_header(small, 0.0, 0.0, call.lags->cdelt1[i3], call.lags->cdelt2[i4], call.lags->crota[i5], call.sem, hc))
        return false;
    build_slots(call.d, c, call.lag_begin, call.lag_end, plan.rects, slots);
    return slots->n_batches > 0;
}

// the affine part of a launch's uniforms (MODE_CAR: pixel <-> native angles); the other members are left as they are
inline void set_affine(LaunchU* u, const Affine2& a) {
    u->m00 = a.m00;
    u->m01 = a.m01;
    u->m10 = a.m10;
    u->m11 = a.m11;
    u->b0 = a.b0;
    u->b1 = a.b1;
}

// ---- the Carrington host tables behind their key ----------------------------------------------------------------------
// Rebuilds `t` when `key` does not describe (g, crln_obs, rot) -- everything the tables depend on, caller-supplied
// latitude trig by value -- or when `force` says so.  True: rebuilt (the device copies are stale).
// rot: differential rotation of the image the tables are for (null: none)
inline bool update_carr_tables(CarrTables& t, std::vector<double>& key, const coreg_carr_grid& g, double crln_obs,
                               const coreg_diffrot* rot, bool force) {
    std::vector<double> k = {g.lon0, g.lon1, (double)g.n_lon, g.lat0, g.lat1, (double)g.n_lat, crln_obs,
                             g.lat_cos ? 1.0 : 0.0, g.lat_sin ? 1.0 : 0.0, rot ? 1.0 : 0.0};
    if (rot) k.insert(k.end(), {rot->delta_t_days, rot->c0, rot->c1, rot->c2});
    if (g.lat_cos) k.insert(k.end(), g.lat_cos, g.lat_cos + g.n_lat);
    if (g.lat_sin) k.insert(k.end(), g.lat_sin, g.lat_sin + g.n_lat);
    if (k == key && !force) return false;
    carr_tables(g, crln_obs, t);
    if (rot) {
        diffrot_dx(t.sin_lat.data(), g.n_lat, *rot, t.dx);
        // nothing to rotate: the per-column tables serve, as without a rotation
        if (std::all_of(t.dx.begin(), t.dx.end(), [](double v) { return v == 0.0; })) t.dx.clear();
    }
    key.swap(k);
    return true;
}

// host mirror of kernels.hpp carr_term (tile-shape heuristics only)
inline bool carr_term_host(const CarrTables& t, const CarrCommon& c, int i, int j, double* t0, double* t1) {
    const double cl = (double)t.cos_lat[j], y = (double)t.sin_lat[j];
    const double x = cl * t.sin_lon[i], z = cl * t.cos_lon[i];
    const double zz = z * c.cb + y * c.sb, yy = y * c.cb - z * c.sb;
    const double yr = yy * c.cr - x * c.sr, xr = x * c.cr + yy * c.sr;
    const double zd = c.dist - zz;
    *t0 = std::atan(xr / zd) * kRad2Deg * 3600.0 / c.cdelt1;
    *t1 = std::atan(yr / zd) * kRad2Deg * 3600.0 / c.cdelt2;
    return zz >= 0.0;
}

// ---- lag-points decided by wcslib's rounding noise --------------------------------------------------------
// Zero-CRVAL lags of a helioprojective sweep share the target header's tangent point, so the map target pixel ->
// shifted pixel is exactly affine, A = (CDELT' PC')^-1 (CDELT PC) about CRPIX.  When A leaves an image axis invariant
// (the zero lag: A = I; a CDELT1-only lag: rows map to rows; CDELT2-only: columns to columns; `reference` CDELT
// semantics: A = I up to the rebuilt PC's last bit) the border rows / columns of the grid sit ON the bounds rule
// c < 0 or c > n-1 and what the reference does with them is decided by the rounding noise of its wcslib round trip
// (alignment.py:1038-1069).  For such a lag the device map is SNAPPED to the exact invariant form (every border
// pixel in bounds along that axis) and the pixels wcslib drops are listed for k_border_fix.
struct AxisInvariance {
    bool rows = false, cols = false;
};
inline AxisInvariance snap_invariant_axes(const coreg_wcs2d& target, const coreg_wcs2d& shifted, int gw, int gh, double hm[9]) {
    AxisInvariance inv;
    if (target.crval1 != shifted.crval1 || target.crval2 != shifted.crval2 || target.lonpole != shifted.lonpole ||
        target.unit_to_deg != shifted.unit_to_deg)
        return inv;
    const Mat3 a = mat_mul(iwc_to_pix(shifted), pix_to_iwc(target));
    const double tol = 1e-6;  // pixels, over the whole grid; rounding noise is < 1e-9, a real lag moves >> 1e-6
    const double a00 = (double)a.m[0][0], a01 = (double)a.m[0][1], a02 = (double)a.m[0][2];
    const double a10 = (double)a.m[1][0], a11 = (double)a.m[1][1], a12 = (double)a.m[1][2];
    inv.rows = std::fabs(a10) * gw + std::fabs(a11 - 1.0) * gh + std::fabs(a12) < tol;
    inv.cols = std::fabs(a00 - 1.0) * gw + std::fabs(a01) * gh + std::fabs(a02) < tol;
    if (inv.rows || inv.cols) {
        hm[0] = inv.cols ? 1.0 : a00;
        hm[1] = inv.cols ? 0.0 : a01;
        hm[2] = inv.cols ? 0.0 : a02;
        hm[3] = inv.rows ? 0.0 : a10;
        hm[4] = inv.rows ? 1.0 : a11;
        hm[5] = inv.rows ? 0.0 : a12;
        hm[6] = hm[7] = 0.0;
        hm[8] = 1.0;
    }
    return inv;
}

// the key of both wcslib caches: the header pair, the shapes and the invariant axes
inline std::vector<double> wcslib_cache_key(const SweepEnv& env, const coreg_wcs2d& target, const coreg_wcs2d& shifted,
                                            AxisInvariance inv) {
    return {(double)target.proj, target.latpole == target.latpole ? target.latpole : -999.0, target.crpix1, target.crpix2, target.crval1, target.crval2, target.cdelt1, target.cdelt2,
            target.pc1_1, target.pc1_2, target.pc2_1, target.pc2_2, target.unit_to_deg,
            target.lonpole == target.lonpole ? target.lonpole : -999.0,
            shifted.crpix1, shifted.crpix2, shifted.cdelt1, shifted.cdelt2, shifted.pc1_1,
            shifted.pc1_2, shifted.pc2_1, shifted.pc2_2, (double)env.gW, (double)env.gH, (double)env.sW,
            (double)env.sH, inv.rows ? 1.0 : 0.0, inv.cols ? 1.0 : 0.0};
}

// Pixels of the invariant border rows / columns that the reference's round trip pixel -> sky (target header) ->
// ang2pipi -> pixel (shifted header) sends outside [0, W-1] x [0, H-1] of the image to align.  Appended to `out`.
template <typename Chain>
void wcslib_dropped_border_pixels_t(const SweepEnv& env, const coreg_wcs2d& target, const coreg_wcs2d& shifted,
                                    AxisInvariance inv, std::vector<int>* out) {
    const int gw = env.gW, gh = env.gH;
    std::vector<double> key = wcslib_cache_key(env, target, shifted, inv);
    auto& cache = env.caches->border;
    auto hit = cache.find(key);
    if (hit == cache.end()) {
        Chain wf, wt;
        wf.init(target);
        wt.init(shifted);
        std::vector<int> cand;  // row-major, each pixel once
        const int jb = env.sH - 1, ib = env.sW - 1;
        for (int j = 0; j < gh; ++j) {
            const bool row = inv.rows && (j == 0 || j == jb);
            if (row) {
                for (int i = 0; i < gw; ++i) cand.push_back(j * gw + i);
            } else if (inv.cols) {
                cand.push_back(j * gw);
                if (ib > 0 && ib < gw) cand.push_back(j * gw + ib);
            }
        }
        std::vector<char> drop(cand.size(), 0);
        const double wmax = (double)(env.sW - 1), hmax = (double)(env.sH - 1);
        auto work = [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; ++k) {
                double x, y;
                wcslib_pixel_to_pixel(wf, wt, (double)(cand[k] % gw), (double)(cand[k] / gw), &x, &y);
                drop[k] = !((x >= 0.0) && (x <= wmax) && (y >= 0.0) && (y <= hmax));  // NaN -> dropped
            }
        };
        parallel_for((long long)cand.size(), cand.size() < 2048 ? 1 : 8, 0, work);
        std::vector<int> dropped;
        for (size_t k = 0; k < cand.size(); ++k)
            if (drop[k]) dropped.push_back(cand[k]);
        if (cache.size() >= 64) cache.clear();
        hit = cache.emplace(std::move(key), std::move(dropped)).first;
    }
    out->insert(out->end(), hit->second.begin(), hit->second.end());
}

inline void wcslib_dropped_border_pixels(const SweepEnv& env, const coreg_wcs2d& target, const coreg_wcs2d& shifted,
                                         AxisInvariance inv, std::vector<int>* out) {
    if (target.proj == COREG_PROJ_CAR) wcslib_dropped_border_pixels_t<WcslibCar>(env, target, shifted, inv, out);
    else wcslib_dropped_border_pixels_t<WcslibTan>(env, target, shifted, inv, out);
}

// Odd spline orders: for every grid pixel, does the reference's round trip come back BELOW the integer along an
// invariant axis (bit 0: rows / y, bit 1: columns / x)?  Then floor(c) -- the first tap of an odd-order spline -- is one
// less than at the exact integer the sweep used (k_parity_fix).  W x H evaluations of the wcslib chain, in threads;
// cached per header pair.
template <typename Chain>
const std::vector<unsigned char>& wcslib_tap_shift_flags_t(const SweepEnv& env, const coreg_wcs2d& target,
                                                           const coreg_wcs2d& shifted, AxisInvariance inv) {
    const int gw = env.gW, gh = env.gH;
    std::vector<double> key = wcslib_cache_key(env, target, shifted, inv);
    auto& cache = env.caches->flags;
    auto hit = cache.find(key);
    if (hit != cache.end()) return hit->second;
    Chain wf, wt;
    wf.init(target);
    wt.init(shifted);
    std::vector<unsigned char> flags((size_t)gw * gh, 0);
    const double wmax = (double)(env.sW - 1), hmax = (double)(env.sH - 1);
    auto work = [&](int j0, int j1) {
        for (int j = j0; j < j1; ++j)
            for (int i = 0; i < gw; ++i) {
                double x, y;
                wcslib_pixel_to_pixel(wf, wt, (double)i, (double)j, &x, &y);
                unsigned char f = 0;
                if (inv.rows && y < (double)j) f |= 1;
                if (inv.cols && x < (double)i) f |= 2;
                // the bounds rule drops the pixel altogether (border pixels only; k_border_fix has taken it out)
                if (!((x >= 0.0) && (x <= wmax) && (y >= 0.0) && (y <= hmax))) f |= 4;
                flags[(size_t)j * gw + i] = f;
            }
    };
    parallel_for(gh, (long long)gw * gh < 4096 ? 1 : 12, 0, work);
    if (cache.size() >= 4) cache.clear();
    return cache.emplace(std::move(key), std::move(flags)).first->second;
}

inline const std::vector<unsigned char>& wcslib_tap_shift_flags(const SweepEnv& env, const coreg_wcs2d& target,
                                                                const coreg_wcs2d& shifted, AxisInvariance inv) {
    if (target.proj == COREG_PROJ_CAR) return wcslib_tap_shift_flags_t<WcslibCar>(env, target, shifted, inv);
    return wcslib_tap_shift_flags_t<WcslibTan>(env, target, shifted, inv);
}

// lag-points of a launch whose border pixels are decided by wcslib's rounding noise: the host side of a BorderFix
struct BorderItems {
    struct Item {
        long long slot;  // slot of the launch
        int first, n;    // its pixels in `pixels` (and in the handle's device copy of them): [first, first + n)
        long long flags_off;  // odd spline order: offset of its per-pixel tap-shift flags in the uploaded flag grids, or -1
    };
    std::vector<Item> items;
    std::vector<int> pixels;  // concatenated linear grid indices
};

// The single-sample pass, host part (between the scan and the upload of host_fix_lists.hpp's prepare_tap_fix): the
// (slot, pixel) samples the scan listed, in whatever order its atomics listed them, grouped by slot (counting sort); every
// segment is put in pixel order by the thread that evaluates it, so the summation order of k_tap_fix does not depend on the
// scan's; and wcslib's chain (`shifted_of(slot)`: the slot's shifted header) gives every sample its coordinates.
struct TapSample {
    unsigned slot, pixel;  // (k_tap_scan's uint2) lag slot of the launch, linear grid index
};
struct TapLists {
    std::vector<int> seg_slot, seg_begin;  // per listed lag-point: its slot, its first entry; seg_begin has one more: the count
    std::vector<unsigned> pixel;           // per entry
    std::vector<double> xw, yw;            // per entry: the sample's coordinates as the reference's round trip returns them
};
template <typename ShiftedOf>
TapLists group_tap_samples(const std::vector<TapSample>& list, long long n_slots, int gw, const coreg_wcs2d& target,
                           ShiftedOf shifted_of) {
    const unsigned count = (unsigned)list.size();
    TapLists t;
    std::vector<int> first((size_t)n_slots + 1, 0);
    for (unsigned k = 0; k < count; ++k) ++first[(size_t)list[k].slot + 1];
    for (long long sl = 0; sl < n_slots; ++sl) first[(size_t)sl + 1] += first[(size_t)sl];
    std::vector<unsigned>& pixel = t.pixel;
    pixel.resize(count);
    {
        std::vector<int> at(first.begin(), first.end() - 1);
        for (unsigned k = 0; k < count; ++k) pixel[(size_t)at[list[k].slot]++] = list[k].pixel;
    }
    std::vector<int>& seg_slot = t.seg_slot;
    std::vector<int>& seg_begin = t.seg_begin;
    for (long long sl = 0; sl < n_slots; ++sl)
        if (first[(size_t)sl + 1] > first[(size_t)sl]) {
            seg_slot.push_back((int)sl);
            seg_begin.push_back(first[(size_t)sl]);
        }
    seg_begin.push_back((int)count);
    const int n_seg = (int)seg_slot.size();
    std::vector<double>& xw = t.xw;
    std::vector<double>& yw = t.yw;
    xw.resize(count);
    yw.resize(count);
    WcslibTan wf;
    WcslibCar wfc;
    const bool car = target.proj == COREG_PROJ_CAR;
    if (car) wfc.init(target);
    else wf.init(target);
    auto work = [&](int s0, int s1) {  // (one segment at a time: the threads share the entries about evenly)
        for (int sg = s0; sg < s1; ++sg) {
            std::sort(pixel.begin() + seg_begin[sg], pixel.begin() + seg_begin[sg + 1]);
            if (car) {
                WcslibCar wt;
                wt.init(shifted_of(seg_slot[sg]));
                for (int e = seg_begin[sg]; e < seg_begin[sg + 1]; ++e)
                    wcslib_pixel_to_pixel(wfc, wt, (double)(pixel[e] % (unsigned)gw), (double)(pixel[e] / (unsigned)gw), &xw[e], &yw[e]);
            } else {
                WcslibTan wt;
                wt.init(shifted_of(seg_slot[sg]));
                for (int e = seg_begin[sg]; e < seg_begin[sg + 1]; ++e)
                    wcslib_pixel_to_pixel(wf, wt, (double)(pixel[e] % (unsigned)gw), (double)(pixel[e] / (unsigned)gw), &xw[e], &yw[e]);
            }
        }
    };
    parallel_for(n_seg, count < 4096 ? 1 : 12, 1, work);
    return t;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------
// One precompute + one sweep launch over n_batches * kBlock slots of the plan, from slot `slot_off` on.
struct PlannedLaunch {
    int mode = MODE_TRANSLATE;  // of the sweep kernel and the single-sample scan (the precompute of either homography
                                // mode is MODE_HOMOGRAPHY's)
    size_t slot_off = 0;
    int n_batches = 0;
    int n_groups = 0;        // tile groups of its precompute (pick_groups)
    bool precompute = true;  // false: the compacted points and the work partition of the launch before it serve as they are
    // the geometry part of PrecomputeArgs
    double f0lo = 0, f0hi = 0, f1lo = 0, f1hi = 0;  // cull box on the base coordinates (inclusive)
    CarrCommon cc = {};                              // MODE_TRANSLATE
    LaunchU car_fwd = {};                            // MODE_CAR: target pixel -> its native angles (zero: pixel indices)
    int tile_skip = 0;                               // MODE_TRANSLATE: the whole-tile skip bound of k_precompute ...
    double lip_x = 0, lip_y = 0, dlon = 0, dlat = 0;  // ... pixels per radian of grid-point motion, grid steps in radians
    LaunchU car_inv = {};      // MODE_CAR: the launch's native -> pixel map, box_c, pole_sep
    bool border_items = false;  // the plan's BorderItems are this launch's
    // The single-sample scan of the launch (scan false: none).  Slot s has the header hc[slot_hc[s]] (slot_hc empty: hc[0])
    // with the CRVAL lags i1[s], i2[s] added to the CRVAL of the header being lagged; skip[s] = 1: not scanned (padding,
    // lag-points the structured fix handles, lag-points that cannot sit on integers).
    bool scan = false;
    std::vector<coreg_wcs2d> hc;
    std::vector<int> slot_hc, i1, i2;
    std::vector<unsigned char> tap_skip;
    double scan_box[4] = {0, 0, 0, 0};  // target pixels scanned: [x0, x1, y0, y1]
};

struct SweepPlan {
    const char* error = nullptr;  // the headers admit no plan (COREG_EINVAL with this message)
    std::vector<double> params;   // per launch, one after another: SoA [2 or 9][slots of the launch]
    std::vector<long long> outidx;  // raveled lag index of every slot, -1: padding
    Plan lags;                    // tile shape and lag patches
    int pitch = 0;                // compile-time LDS window pitch of the sweep launches, 0: per visit
    std::vector<PlannedLaunch> launches;  // none: every lag-point of the call is NaN
    BorderItems fix;
    std::vector<std::vector<unsigned char>> flags;  // per noise-decided lag-point (odd spline orders): one grid of tap-shift flags
    coreg_wcs2d target = {};        // the single-sample scans: the target header ...
    double crval1 = 0, crval2 = 0;  // ... and the CRVAL of the header being lagged (shifted_of)
    bool empty() const { return launches.empty(); }
    // the shifted header of slot `slot` of launch L, as its single-sample scan needs it
    coreg_wcs2d shifted_of(const PlannedLaunch& L, const coreg_lags& lags_, int slot) const {
        coreg_wcs2d hl = L.hc[L.slot_hc.empty() ? 0 : (size_t)L.slot_hc[(size_t)slot]];
        hl.crval1 = crval1 + lags_.crval1[L.i1[(size_t)slot]];  // alignment.py:404
        hl.crval2 = crval2 + lags_.crval2[L.i2[(size_t)slot]];  // alignment.py:412
        return hl;
    }
};

// ---- Carrington: every (cdelt1, cdelt2, crota) combination = one precompute + one sweep launch --------------------------
// env.tabs: the host tables of `grid` under hdr_small's CRLN_OBS (update_carr_tables).
inline SweepPlan plan_carrington(const SweepCall& call, const coreg_wcs2d& hdr_small, const coreg_carr_grid& grid,
                                 double solar_r, const SweepEnv& env) {
    const coreg_lags* lags = call.lags;
    const LagDims& d = call.d;
    const CarrTables& tabs = *env.tabs;
    SweepPlan sp;
    // differential rotation: neighbouring rows slide against each other by up to this many radians of longitude, which
    // the whole-tile bound below adds to the per-row step
    double row_slip = 0.0;
    for (size_t j = 1; j < tabs.dx.size(); ++j) row_slip = std::max(row_slip, std::fabs(tabs.dx[j] - tabs.dx[j - 1]));
    row_slip *= kDeg2Rad * (1.0 + 1e-9);

    // local geometry (heuristic inputs only) -> tile shape + lag patch
    Geometry geo;
    {
        const CarrCommon c0 = carr_common(hdr_small, solar_r);
        const int ic = grid.n_lon / 2, jc = grid.n_lat / 2;
        double a0, a1, b0, b1, c0x, c0y;
        carr_term_host(tabs, c0, ic, jc, &a0, &a1);
        carr_term_host(tabs, c0, std::min(ic + 1, grid.n_lon - 1), jc, &b0, &b1);
        carr_term_host(tabs, c0, ic, std::min(jc + 1, grid.n_lat - 1), &c0x, &c0y);
        geo.dx_di = b0 - a0;
        geo.dy_di = b1 - a1;
        geo.dx_dj = c0x - a0;
        geo.dy_dj = c0y - a1;
        // utils/rectify.py:399-404: X0 = -(c d1 + s d2)/cdelt1, Y0 = -(-s d1 + c d2)/cdelt2
        const double s1 = lag_step(lags->crval1, d.n1), s2 = lag_step(lags->crval2, d.n2);
        geo.ax = c0.cr * s1 / hdr_small.cdelt1;
        geo.ay = c0.sr * s1 / hdr_small.cdelt2;
        geo.bx = c0.sr * s2 / hdr_small.cdelt1;
        geo.by = c0.cr * s2 / hdr_small.cdelt2;
    }
    sp.lags = plan_lags(env, geo, call);
    sp.pitch = pick_pitch(env.pitch, env.use_lds, sp.lags, env.use_lds ? env.lds_elems : 0, call.order);

    // all lag parameters of all launches are staged together: per launch [X0 x ns][Y0 x ns]
    std::vector<double>& params = sp.params;
    std::vector<long long>& outidx = sp.outidx;
    SlotList slots;
    for (long long c = 0; c < d.nc; ++c) {
        coreg_wcs2d hc;
        if (!combo_slots(call, hdr_small, sp.lags, c, &hc, &slots)) continue;
        const size_t ns = slots.i1.size();
        PlannedLaunch L;
        L.mode = MODE_TRANSLATE;
        L.slot_off = outidx.size();
        L.n_batches = slots.n_batches;
        L.n_groups = pick_groups(env.shard_world, env.n_groups, L.n_batches);
        L.cc = carr_common(hc, solar_r);
        const size_t pbase = params.size();
        params.resize(pbase + 2 * ns);
        double x0min = 1e300, x0max = -1e300, y0min = 1e300, y0max = -1e300;
        // utils/rectify.py:396-404 with the roll trig hoisted out of the per-lag loop (same values, same order)
        const double roll = hc.crota * kDeg2Rad;
        const double rc = std::cos(roll), rs = std::sin(roll);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t s = 0; s < ns; ++s) {
            // padding lanes get NaN: they fail the bounds rule for every point, so waves made only of padding
            // skip every point with one branch (their slots are never written by k_finalize)
            if (slots.outidx[s] < 0) {
                params[pbase + s] = nan;
                params[pbase + ns + s] = nan;
                continue;
            }
            const double v1 = hdr_small.crval1 + lags->crval1[slots.i1[s]];  // alignment.py:404
            const double v2 = hdr_small.crval2 + lags->crval2[slots.i2[s]];  // alignment.py:412
            const double dx = rc * v1 + rs * v2;
            const double dy = -rs * v1 + rc * v2;
            // (never -0.0: a difference whose minuend, itself a difference, is not -0.0 -- k_sweep's bounded loop tests
            // the bounds rule on the bit pattern of X0 + t0 and relies on it, kernels_sweep.hpp point_lag)
            const double x0 = (hc.crpix1 - 1) - dx / hc.cdelt1;
            const double y0 = (hc.crpix2 - 1) - dy / hc.cdelt2;
            params[pbase + s] = x0;
            params[pbase + ns + s] = y0;
            x0min = std::min(x0min, x0);
            x0max = std::max(x0max, x0);
            y0min = std::min(y0min, y0);
            y0max = std::max(y0max, y0);
        }
        outidx.insert(outidx.end(), slots.outidx.begin(), slots.outidx.end());
        // a point can be in bounds for some lag only if X0 + t0 in [0, W-1] for some X0 in [x0min, x0max]
        L.f0lo = -x0max;
        L.f0hi = (double)(env.sW - 1) - x0min;
        L.f1lo = -y0max;
        L.f1hi = (double)(env.sH - 1) - y0min;
        // whole-tile skip bound (k_precompute): pixels per radian of grid-point motion, grid steps in radians
        const double dm1 = L.cc.dist - 1.0;
        L.tile_skip = (env.tile_skip && dm1 > 0.0) ? 1 : 0;
        const double per_rad = L.tile_skip ? (1.0 / dm1 + 1.0 / (dm1 * dm1)) * kRad2Deg * 3600.0 : 0.0;
        L.lip_x = per_rad / std::fabs(L.cc.cdelt1) * (1.0 + 1e-9);
        L.lip_y = per_rad / std::fabs(L.cc.cdelt2) * (1.0 + 1e-9);
        // float32 linspace grid: the spacing is uniform to ~1e-7 relative of the coordinate
        L.dlon = grid.n_lon > 1 ? (std::fabs(grid.lon1 - grid.lon0) / (grid.n_lon - 1) * 1.001 + 1e-4) * kDeg2Rad : 0.0;
        L.dlat = grid.n_lat > 1 ? (std::fabs(grid.lat1 - grid.lat0) / (grid.n_lat - 1) * 1.001 + 1e-4) * kDeg2Rad : 0.0;
        L.dlat += row_slip;
        sp.launches.push_back(std::move(L));
    }
    return sp;
}

// ---- plate-carree maps on both sides ----------------------------------------------------------------------------------
// (Alignment.align_using_initial_carrington, alignment.py:344-399 -> _interpolate_on_large_data_grid :1018-1029 with
// WCS(CRLN-CAR)): the per-lag map is a rotation of the sphere between the native frames of the two maps (a CRVAL2 lag
// makes the shifted map oblique).  One precompute (native angles of the target pixels), one sweep launch per (cdelt1,
// cdelt2, crota) combination (its native -> pixel affine map is a launch constant).  Lags whose header has no valid
// native pole get NaN (astropy raises for them).
inline bool same_header(const coreg_wcs2d& a, const coreg_wcs2d& b) {
    auto eq = [](double x, double y) { return x == y || (x != x && y != y); };
    return a.proj == b.proj && a.crpix1 == b.crpix1 && a.crpix2 == b.crpix2 && a.crval1 == b.crval1 &&
           a.crval2 == b.crval2 && a.cdelt1 == b.cdelt1 && a.cdelt2 == b.cdelt2 && a.pc1_1 == b.pc1_1 &&
           a.pc1_2 == b.pc1_2 && a.pc2_1 == b.pc2_1 && a.pc2_2 == b.pc2_2 && a.unit_to_deg == b.unit_to_deg &&
           eq(a.lonpole, b.lonpole) && eq(a.latpole, b.latpole) && a.naxis1 == b.naxis1 && a.naxis2 == b.naxis2;
}

// The launch of the identity lag-point `identity_out` (plan_car: taken out of its combination's launch), appended to
// the plan: one batch, one live slot with the identity homography (every sample ON its pixel), the others padding.
// Target pixel -> the same pixel of the map to align: base coordinates = pixel indices (car_fwd zero), no culling by
// position.  (It is the sweep's last launch: no MODE_CAR launch finds its points, which hold pixel indices and not unit
// vectors.)  Its border pixels and, at odd orders, its tap sets are what wcslib's chain decides.
inline void add_identity_launch(int order, const coreg_wcs2d& hdr_target, const SweepEnv& env, long long identity_out,
                                SweepPlan* plan) {
    SweepPlan& sp = *plan;
    const double nanv = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    PlannedLaunch L;
    L.mode = MODE_HOMOGRAPHY;
    L.slot_off = sp.outidx.size();
    L.n_batches = 1;
    L.n_groups = pick_groups(env.shard_world, env.n_groups, 1);
    L.f0lo = L.f1lo = -inf;
    L.f0hi = L.f1hi = inf;
    L.border_items = true;
    const size_t ns = kBlock, pbase = sp.params.size();
    sp.params.resize(pbase + 9 * ns, nanv);
    const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) sp.params[pbase + (size_t)k * ns] = ident[k];
    sp.outidx.push_back(identity_out);
    sp.outidx.insert(sp.outidx.end(), ns - 1, -1);
    sp.launches.push_back(std::move(L));
    // (on every rank of a grid-sharded sweep: launch_sweep applies it on rank 0 only, but all must agree that this
    // launch carries a correction)
    AxisInvariance inv;
    inv.rows = inv.cols = true;
    BorderItems::Item it;
    it.slot = 0;
    it.first = 0;
    wcslib_dropped_border_pixels(env, hdr_target, hdr_target, inv, &sp.fix.pixels);
    it.n = (int)sp.fix.pixels.size();
    it.flags_off = -1;
    if (order & 1) {
        it.flags_off = 0;
        sp.flags.push_back(wcslib_tap_shift_flags(env, hdr_target, hdr_target, inv));
    }
    if (it.n > 0 || it.flags_off >= 0) sp.fix.items.push_back(it);
}

inline SweepPlan plan_car(const SweepCall& call, const coreg_wcs2d& hdr_target, const coreg_wcs2d& hdr_small,
                          const SweepEnv& env) {
    const coreg_lags* lags = call.lags;
    const LagDims& d = call.d;
    SweepPlan sp;
    sp.target = hdr_target;
    sp.crval1 = hdr_small.crval1;
    sp.crval2 = hdr_small.crval2;
    Mat3 r_target;
    if (car_native_to_celestial(hdr_target, &r_target)) {
        sp.error = "hdr_target: no valid native pole for this CRVAL2 / LONPOLE (CAR)";
        return sp;
    }
    auto shifted_by = [&](const coreg_wcs2d& base, double v1, double v2) {
        coreg_wcs2d hl = base;
        hl.crval1 = hdr_small.crval1 + v1;  // alignment.py:404
        hl.crval2 = hdr_small.crval2 + v2;  // alignment.py:412
        return hl;
    };
    auto shifted = [&](const coreg_wcs2d& base, int i1, int i2) {
        return shifted_by(base, lags->crval1[i1], lags->crval2[i2]);
    };
    sp.lags = plan_lags(env, local_geometry(hdr_target, call, [&](double v1, double v2, double u, double v,
                                                                  double* x, double* y) {
        CarMapHost m;
        if (m.init(hdr_target, shifted_by(hdr_small, v1, v2))) return false;
        m.apply(u, v, x, y);
        return true;
    }), call);
    const Plan& plan = sp.lags;

    // rotation of every (CRVAL1, CRVAL2) lag: R = R_small(lag)^T * R_target  (PC / CDELT do not enter it)
    const int i1_lo = call.i1_lo(), i1_hi = call.i1_hi();
    std::vector<double> rot((size_t)(i1_hi - i1_lo + 1) * d.n2 * 9);
    const double nanv = std::numeric_limits<double>::quiet_NaN();
    for (int i1 = i1_lo; i1 <= i1_hi; ++i1)
        for (int i2 = 0; i2 < d.n2; ++i2) {
            double* r = &rot[((size_t)(i1 - i1_lo) * d.n2 + i2) * 9];
            Mat3 rs;
            if (car_native_to_celestial(shifted(hdr_small, i1, i2), &rs)) {
                for (int k = 0; k < 9; ++k) r[k] = nanv;
                continue;
            }
            const Mat3 m = mat_mul(mat_T(rs), r_target);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) r[3 * a + b] = (double)m.m[a][b];
        }

    std::vector<double>& params = sp.params;  // per launch: SoA [9][slots of the launch]
    std::vector<long long>& outidx = sp.outidx;
    SlotList slots;
    const bool same_shape = env.gW == env.sW && env.gH == env.sH;
    const double inf = std::numeric_limits<double>::infinity();
    // The identity lag-point (shifted header == target header: the zero lag of the sub-map semantics, where the target IS
    // the header of the map to align).  The reference's pixel -> world -> pixel round trip (alignment.py:1038-1069) returns
    // i + eps there and the sign of wcslib's rounding noise decides the bounds rule on every border pixel (and, for odd
    // spline orders, the tap set of every pixel).  The sphere rotation of this path cannot even return exact integers, so
    // that lag-point is taken out of the CAR launch and swept on its own with the EXACT identity map by the
    // helioprojective kernels, whose zero-lag machinery (k_border_fix / k_parity_fix) then applies what wcslib's chain
    // (geometry.hpp WcslibCar, bit-exact) decides.  "border_fix" 0: rotation path for that lag-point too.
    long long identity_out = -1;
    for (long long c = 0; c < d.nc; ++c) {
        coreg_wcs2d hc;
        if (!combo_slots(call, hdr_small, plan, c, &hc, &slots)) continue;
        const size_t ns = slots.i1.size();
        PlannedLaunch L;
        L.mode = MODE_CAR;
        L.slot_off = outidx.size();
        L.n_batches = slots.n_batches;
        L.n_groups = pick_groups(env.shard_world, env.n_groups, L.n_batches);
        set_affine(&L.car_fwd, car_pix_to_native(hdr_target));
        L.f0lo = L.f1lo = -inf;  // no culling by position: only non-finite reference values drop out
        L.f0hi = L.f1hi = inf;
        set_affine(&L.car_inv, car_native_to_pix(hc));
        L.car_inv.box_c = car_box_c(hdr_target, hc, plan.tile_w);
        L.car_inv.pole_sep = 0.0;  // largest over the lags of this launch (below)
        const size_t pbase = params.size();
        params.resize(pbase + 9 * ns);
        // the single-sample pass of this launch skips all slots but the lags that leave CRVAL1 or CRVAL2 of the
        // target header alone: only those bring whole rows or columns of coordinates (or, with a CROTA / CDELT lag on top,
        // the reference pixel) back within wcslib's noise of integers
        L.tap_skip.reserve(ns);
        for (size_t s = 0; s < ns; ++s) {
            bool pad = slots.outidx[s] < 0;
            if (!pad && env.border_fix && identity_out < 0 && same_shape) {
                const coreg_wcs2d hl = shifted(hc, slots.i1[s], slots.i2[s]);
                if (same_header(hl, hdr_target)) {
                    identity_out = slots.outidx[s];
                    slots.outidx[s] = -1;  // not this launch's: padding lane (NaN map, nothing written)
                    pad = true;
                }
            }
            const double* r = &rot[((size_t)(slots.i1[s] - i1_lo) * d.n2 + slots.i2[s]) * 9];
            for (int k = 0; k < 9; ++k) params[pbase + (size_t)k * ns + s] = pad ? nanv : r[k];
            if (!pad && r[8] == r[8]) L.car_inv.pole_sep = std::max(L.car_inv.pole_sep, car_pole_sep(r));
            unsigned char skip = 1;
            if (!pad && env.tap_fix && r[8] == r[8] && same_shape) {
                // (a CROTA / CDELT lag on top of it included: with both CRVAL equal the map is affine about CRPIX and
                // returns the reference pixel itself to within the noise)
                const coreg_wcs2d hl = shifted(hc, slots.i1[s], slots.i2[s]);
                if (hl.crval1 == hdr_target.crval1 || hl.crval2 == hdr_target.crval2) skip = 0;
            }
            L.tap_skip.push_back(skip);
            L.scan = L.scan || !skip;
        }
        L.hc.push_back(hc);
        L.i1 = slots.i1;
        L.i2 = slots.i2;
        L.scan_box[1] = (double)(env.gW - 1);
        L.scan_box[3] = (double)(env.gH - 1);
        outidx.insert(outidx.end(), slots.outidx.begin(), slots.outidx.end());
        sp.launches.push_back(std::move(L));
    }
    // the work partition (k_tile_list) depends on the group count of the launch: redo it only when that changes
    int last_groups = -1, last_batches = -1;
    for (PlannedLaunch& L : sp.launches) {
        L.precompute = L.n_groups != last_groups || L.n_batches != last_batches;
        last_groups = L.n_groups;
        last_batches = L.n_batches;
    }
    if (identity_out >= 0) add_identity_launch(call.order, hdr_target, env, identity_out, &sp);
    if (!sp.empty()) trace("sweep_helioprojective: lane parameters laid out");
    return sp;
}

// ---- helioprojective (TAN): all slots of all (cdelt1, cdelt2, crota) combinations -> ONE launch -----------------------
// Two passes.  (1) per combination, independent of every other and of the caches -- a few host threads share them
// when the lag set is large (cfg4: 21 combinations x 3 721 lag-points, 1.4 ms of 3 x 3 products on one core):
// shifted header, slots, one homography per slot, the combination's corner of the cull box.  (2) in combination
// order, on this thread: the lag-points decided by wcslib's rounding noise (the caches), the bookkeeping of the
// single-sample pass, the concatenation.
struct TanCombo {
    bool used = false;
    coreg_wcs2d hc;
    SlotList slots;
    std::vector<double> hs;  // AoS [slot][9]
    double box[4] = {1e300, -1e300, 1e300, -1e300};
};

// Pass 1 for combination c.  Its corner of the cull box -- which target pixels can ever be in bounds: inverse maps of the
// small image's corners for the lags on the boundary of the (CRVAL1, CRVAL2) rectangle, chosen BY VALUE (the reference
// accepts lag lists in any order): e1 / e2 = smallest, most central and largest value of each axis (extreme_lags; e1 counts
// from i1_lo) -- the maps vary smoothly and monotonically with the lag value, the +-3 px margin of the launch covers the
// curvature in between.
inline void plan_tan_combo(const SweepCall& call, const coreg_wcs2d& hdr_target, const coreg_wcs2d& hdr_small,
                           const SweepEnv& env, const Plan& plan, const HomographyFamily& fam, int i1_lo, const int e1[3],
                           const int e2[3], long long c, TanCombo* out) {
    const coreg_lags* lags = call.lags;
    TanCombo& cp = *out;
    cp.used = combo_slots(call, hdr_small, plan, c, &cp.hc, &cp.slots);
    if (!cp.used) return;
    const double nanv = std::numeric_limits<double>::quiet_NaN();
    const Mat3d B = HomographyFamily::combo(cp.hc);
    const size_t n = cp.slots.i1.size();
    cp.hs.resize(9 * n);
    for (size_t s = 0; s < n; ++s) {
        double* hm = &cp.hs[9 * s];
        if (cp.slots.outidx[s] < 0) {  // padding lane: NaN map -> never in bounds
            for (int k = 0; k < 9; ++k) hm[k] = nanv;
        } else {
            fam.get(B, cp.slots.i1[s], cp.slots.i2[s], hm);
        }
    }
    for (int a1 = 0; a1 < 3; ++a1)
        for (int a2 = 0; a2 < 3; ++a2) {
            coreg_wcs2d hl = cp.hc;
            hl.crval1 = hdr_small.crval1 + lags->crval1[i1_lo + e1[a1]];
            hl.crval2 = hdr_small.crval2 + lags->crval2[e2[a2]];
            double hi[9];
            homography(hl, hdr_target, hi);
            for (int k = 0; k < 4; ++k) {
                double px, py;
                apply_h(hi, (k & 1) ? (double)(env.sW - 1) : 0.0, (k & 2) ? (double)(env.sH - 1) : 0.0, &px, &py);
                cp.box[0] = std::min(cp.box[0], px);
                cp.box[1] = std::max(cp.box[1], px);
                cp.box[2] = std::min(cp.box[2], py);
                cp.box[3] = std::max(cp.box[3], py);
            }
        }
}

// Pass 2 for one combination whose slots begin at slot `base` of the launch: the lag-points on the target's tangent point
// (sub-map path, zero CRVAL lag) with an invariant image axis get the exact invariant map on the device and their border
// pixels decided as the reference's wcslib round trip decides them (geometry.hpp WcslibTan, k_border_fix).  `skip`: the
// launch's skip bytes (null: no single-sample pass).
inline void decide_tan_noise(const SweepCall& call, const coreg_wcs2d& hdr_target, const coreg_wcs2d& hdr_small,
                             const SweepEnv& env, TanCombo& cp, size_t base, SweepPlan* sp, std::vector<unsigned char>* skip) {
    const coreg_lags* lags = call.lags;
    const SlotList& slots = cp.slots;
    BorderItems& fix = sp->fix;
    for (size_t s = 0; s < slots.i1.size(); ++s) {
        if (slots.outidx[s] < 0) continue;
        // (the tangent points are compared first: every other lag-point is dismissed without building its header)
        const double v1 = hdr_small.crval1 + lags->crval1[slots.i1[s]];
        const double v2 = hdr_small.crval2 + lags->crval2[slots.i2[s]];
        if (v1 != hdr_target.crval1 || v2 != hdr_target.crval2) continue;
        coreg_wcs2d hl = cp.hc;
        hl.crval1 = v1;
        hl.crval2 = v2;
        double* hm = &cp.hs[9 * s];
        const AxisInvariance inv = snap_invariant_axes(hdr_target, hl, env.gW, env.gH, hm);
        if (!inv.rows && !inv.cols) continue;
        BorderItems::Item it;
        it.slot = (long long)(base + s);
        it.first = (int)fix.pixels.size();
        wcslib_dropped_border_pixels(env, hdr_target, hl, inv, &fix.pixels);
        it.n = (int)fix.pixels.size() - it.first;
        it.flags_off = -1;
        if (call.order & 1) {
            it.flags_off = (long long)sp->flags.size() * env.gW * env.gH;
            sp->flags.push_back(wcslib_tap_shift_flags(env, hdr_target, hl, inv));  // (copy: the cache may evict)
        }
        if (it.n > 0 || it.flags_off >= 0) fix.items.push_back(it);
        if (skip) (*skip)[(size_t)it.slot] = 1;  // (its whole grid sits on integers: k_parity_fix)
    }
}

// AoS per combination -> SoA [9][ns] of the launch, on `threads` threads over the combinations.  Returns eps_max: the
// largest |h6 x + h7 y| over the target grid and all lags.
inline double transpose_tan_params(const std::vector<TanCombo>& cps, unsigned threads, const SweepEnv& env, size_t ns,
                                   std::vector<double>* params_out) {
    std::vector<double>& params = *params_out;
    const long long nc = (long long)cps.size();
    std::vector<size_t> off((size_t)nc + 1, 0);
    for (long long c = 0; c < nc; ++c) off[(size_t)c + 1] = off[(size_t)c] + (cps[(size_t)c].used ? cps[(size_t)c].slots.i1.size() : 0);
    std::vector<double> eps_of((size_t)nc, 0.0);
    auto transpose = [&](long long c) {
        const TanCombo& cp = cps[(size_t)c];
        if (!cp.used) return;
        const size_t n = cp.slots.i1.size(), at = off[(size_t)c];
        double em = 0.0;
        for (size_t s = 0; s < n; ++s) {
            const double* hm = &cp.hs[9 * s];
            for (int k = 0; k < 9; ++k) params[(size_t)k * ns + at + s] = hm[k];
            const double e = std::fabs(hm[6]) * (double)env.gW + std::fabs(hm[7]) * (double)env.gH;
            if (e == e) em = std::max(em, e);
        }
        eps_of[(size_t)c] = em;
    };
    parallel_for(nc, threads, 1, [&](long long lo, long long hi) {
        for (long long c = lo; c < hi; ++c) transpose(c);
    });
    double eps_max = 0.0;
    for (double e : eps_of) eps_max = std::max(eps_max, e);
    return eps_max;
}

inline SweepPlan plan_tan(const SweepCall& call, const coreg_wcs2d& hdr_target, const coreg_wcs2d& hdr_small,
                          const SweepEnv& env) {
    const coreg_lags* lags = call.lags;
    const LagDims& d = call.d;
    SweepPlan sp;
    sp.target = hdr_target;
    sp.crval1 = hdr_small.crval1;
    sp.crval2 = hdr_small.crval2;
    sp.lags = plan_lags(env, local_geometry(hdr_target, call, [&](double v1, double v2, double u, double v,
                                                                  double* x, double* y) {
        coreg_wcs2d hl = hdr_small;
        hl.crval1 = hdr_small.crval1 + v1;
        hl.crval2 = hdr_small.crval2 + v2;
        double hm[9];
        homography(hdr_target, hl, hm);
        apply_h(hm, u, v, x, y);
        return true;
    }), call);
    const Plan& plan = sp.lags;

    HomographyFamily fam;
    fam.init(hdr_target, hdr_small, lags->crval1, d.n1, lags->crval2, d.n2, d.nc > 1);
    const int i1_lo = call.i1_lo(), i1_hi = call.i1_hi();
    fam.fill_products(i1_lo, i1_hi);  // (read-only from here on: `get` is safe to call from several threads)
    int e1[3], e2[3];
    extreme_lags(lags->crval1 + i1_lo, i1_hi - i1_lo + 1, e1);
    extreme_lags(lags->crval2, d.n2, e2);
    std::vector<TanCombo> cps((size_t)d.nc);
    trace("sweep_helioprojective: geometry + lag family ready");
    const unsigned plan_threads =
        env.plan_threads ? env.plan_threads : ((d.nc >= 2 && (long long)d.nc * d.n1 * d.n2 >= 16384) ? 8u : 1u);
    parallel_for(d.nc, plan_threads, 1, [&](long long lo, long long hi) {
        for (long long c = lo; c < hi; ++c) plan_tan_combo(call, hdr_target, hdr_small, env, plan, fam, i1_lo, e1, e2, c, &cps[(size_t)c]);
    });

    // The single-sample pass: what it needs to rebuild a slot's shifted header -- the launch's hc: the (cdelt, crota)-shifted
    // header of each combination; its tap_skip: padding lanes and lag-points the structured fix handles.
    // (grid shares across GPUs: every rank lists the samples -- the re-evaluation of a flagged lag-point needs them on
    // every rank; the correction itself is launched on rank 0 only, launch_sweep)
    // Odd orders: every sample within 1e-8 px of an integer coordinate (the sign of wcslib's noise picks the taps); even
    // orders: only those within 1e-8 px of a BOUND of the image (the sign decides the bounds rule) -- a pure CRVAL1 or
    // CRVAL2 lag under an unrotated header keeps whole border rows / columns of the grid there.
    const bool tap_fixing = env.tap_fix;
    PlannedLaunch L;
    std::vector<long long>& outidx = sp.outidx;
    int n_batches = 0;
    double fx0 = 1e300, fx1 = -1e300, fy0 = 1e300, fy1 = -1e300;  // cull box in target pixels
    for (long long c = 0; c < d.nc; ++c) {
        TanCombo& cp = cps[(size_t)c];
        if (!cp.used) continue;
        const SlotList& slots = cp.slots;
        if (tap_fixing) {
            L.hc.push_back(cp.hc);
            for (size_t s = 0; s < slots.i1.size(); ++s) {
                L.slot_hc.push_back((int)L.hc.size() - 1);
                L.i1.push_back(slots.outidx[s] < 0 ? 0 : slots.i1[s]);
                L.i2.push_back(slots.outidx[s] < 0 ? 0 : slots.i2[s]);
                L.tap_skip.push_back(slots.outidx[s] < 0 ? 1 : 0);
            }
        }
        if (env.border_fix) decide_tan_noise(call, hdr_target, hdr_small, env, cp, outidx.size(), &sp, tap_fixing ? &L.tap_skip : nullptr);
        fx0 = std::min(fx0, cp.box[0]);
        fx1 = std::max(fx1, cp.box[1]);
        fy0 = std::min(fy0, cp.box[2]);
        fy1 = std::max(fy1, cp.box[3]);
        outidx.insert(outidx.end(), slots.outidx.begin(), slots.outidx.end());
        n_batches += slots.n_batches;
    }
    if (n_batches == 0) return sp;
    trace("sweep_helioprojective: combinations planned");
    const size_t ns = outidx.size();
    sp.params.resize(9 * ns);
    const double eps_max = transpose_tan_params(cps, plan_threads, env, ns, &sp.params);
    // 1/(1 + eps) = 1 - eps + eps^2 is exact to float64 below ~4e-6 (eps^3 < 1e-16); wider fields divide exactly
    L.mode = (env.h_series && eps_max < 4.0e-6) ? MODE_HOMOGRAPHY_SERIES : MODE_HOMOGRAPHY;
    L.slot_off = 0;
    L.n_batches = n_batches;
    L.n_groups = pick_groups(env.shard_world, env.n_groups, n_batches);
    // the maps are projective and the image corners bound its interior
    L.f0lo = std::floor(fx0) - 3.0;
    L.f0hi = std::ceil(fx1) + 3.0;
    L.f1lo = std::floor(fy0) - 3.0;
    L.f1hi = std::ceil(fy1) + 3.0;
    L.border_items = true;
    L.scan = tap_fixing;
    L.scan_box[0] = L.f0lo;
    L.scan_box[1] = L.f0hi;
    L.scan_box[2] = L.f1lo;
    L.scan_box[3] = L.f1hi;
    sp.pitch = pick_pitch(env.pitch, env.use_lds, plan, env.use_lds ? env.lds_elems : 0, call.order);
    sp.launches.push_back(std::move(L));
    return sp;
}

}  // namespace coreg
