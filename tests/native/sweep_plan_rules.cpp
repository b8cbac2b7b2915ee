// The planners of the header-shift sweeps (csrc/sweep_plan.hpp) on the host, plain and under sanitizers.  What is checked
// is stated here on its own, not taken from the planners:
//   * slot coverage (all three planners): every lag index of [lag_begin, lag_end) whose header can be shifted appears
//     exactly once in outidx over all launches, every other entry is -1, a launch holds n_batches * 256 slots, the
//     slot_off values are contiguous -- for slices that begin and end mid-row, a slice of one lag-point, an empty slice, a
//     combination range of one combination, lag lists in descending and shuffled order, a CDELT1 lag that cancels CDELT1;
//   * Carrington: X0, Y0 of a live slot are the rectify formula (utils/rectify.py:396-404) evaluated here, padding lanes
//     are NaN, and the cull box is exactly (-x0max, (sW - 1) - x0min, -y0max, (sH - 1) - y0min) over the live slots;
//   * CAR to CAR: the identity lag-point leaves its combination's launch exactly when border_fix is on, the shapes are
//     equal and the shifted header equals the target's field by field (NaN == NaN), at most once, into a launch of its own
//     (one batch, slot 0 the identity map, 255 padding slots); a slot's skip byte is 0 exactly when it is live, its rotation
//     valid, tap_fix on, the shapes equal and the shifted CRVAL1 or CRVAL2 the target's; a lag without a native pole has
//     NaN parameters and stays out of pole_sep;
//   * TAN: the planned homography of every live slot agrees with geometry.hpp's homography(target, shifted) on the four
//     grid corners and the centre to 1e-6 px (the bound tests/native/fuzz_geometry.cpp holds the family to); a slot on the
//     target's tangent point with an invariant axis carries a BorderFix item whose pixels are those an independent loop
//     over the border rows / columns finds dropped, and its skip byte is 1; the sweep mode is the series form exactly when
//     eps_max < 4e-6, for lag sets a factor of 10 to either side;
//   * determinism: the same request planned twice, and on 1 and on 8 threads, gives byte-equal params and outidx;
//   * the single-sample lists (group_tap_samples): one segment per listed slot, slots and pixels ascending, every sample
//     once, coordinates those of wcslib's round trip; the wcslib caches hold at most 64 and 4 entries, cleared when full.
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../euispice_coreg_amd/csrc/sweep_plan.hpp"

using namespace coreg;

namespace {
int n_bad = 0, n_checked = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        ++n_checked;                           \
        if (!(cond)) {                         \
            ++n_bad;                           \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
        }                                      \
    } while (0)

const double kNaN = std::numeric_limits<double>::quiet_NaN();

// ---- requests ---------------------------------------------------------------------------------------------------------
struct Lags {
    std::vector<double> v[5];
    coreg_lags c;
    Lags(std::vector<double> a1, std::vector<double> a2, std::vector<double> a3, std::vector<double> a4, std::vector<double> a5) {
        v[0] = a1; v[1] = a2; v[2] = a3; v[3] = a4; v[4] = a5;
        c.crval1 = v[0].data(); c.n_crval1 = (int)v[0].size();
        c.crval2 = v[1].data(); c.n_crval2 = (int)v[1].size();
        c.cdelt1 = v[2].data(); c.n_cdelt1 = (int)v[2].size();
        c.cdelt2 = v[3].data(); c.n_cdelt2 = (int)v[3].size();
        c.crota = v[4].data(); c.n_crota = (int)v[4].size();
    }
    Lags(const Lags&) = delete;
    long long combos() const { return (long long)(v[2].size() * v[3].size() * v[4].size()); }
};

// the call open_sweep would hand the planner: combinations [c0, c0 + nc) (nc 0: all), slice [begin, end) (end < 0: all)
SweepCall make_call(const Lags& l, long long begin, long long end, long long c0, long long nc, int order, int sem) {
    SweepCall call;
    call.lags = &l.c;
    call.d.n1 = l.c.n_crval1;
    call.d.n2 = l.c.n_crval2;
    call.d.n3 = l.c.n_cdelt1;
    call.d.n4 = l.c.n_cdelt2;
    call.d.n5 = l.c.n_crota;
    call.d.c0 = c0;
    call.d.nc = nc > 0 ? nc : l.combos();
    call.order = order;
    call.method = COREG_METHOD_CORRELATION;
    call.sem = sem;
    call.lag_begin = begin;
    call.lag_end = end < 0 ? call.d.total() : end;
    call.n_out = call.lag_end - call.lag_begin;
    return call;
}

// what planning may read and update, as host_plan.hpp's sweep_env fills it from a handle with default options
struct Bench {
    WcslibCaches caches;
    PlanMemo memo;
    CarrTables tabs;
    std::vector<double> tabs_key;
    SweepEnv env;
    Bench(int sW, int sH, int gW, int gH) {
        env.sW = sW;
        env.sH = sH;
        env.gW = gW;
        env.gH = gH;
        env.lds_elems = 159 * 1024 / 8;
        env.tabs = &tabs;
        env.caches = &caches;
        env.memo = &memo;
    }
    Bench(const Bench&) = delete;
};

// a lag index of the call, unraveled: C order over (CRVAL1, CRVAL2, combination of the range), the combination over
// (CDELT1, CDELT2, CROTA) of the whole lag set
struct LagPoint {
    int i1, i2, i3, i4, i5;
    double d[5];
};
LagPoint lag_point(const SweepCall& call, long long idx) {
    const coreg_lags& l = *call.lags;
    LagPoint p;
    const long long g = idx % call.d.nc + call.d.c0;
    p.i2 = (int)((idx / call.d.nc) % l.n_crval2);
    p.i1 = (int)(idx / (call.d.nc * l.n_crval2));
    p.i5 = (int)(g % l.n_crota);
    p.i4 = (int)((g / l.n_crota) % l.n_cdelt2);
    p.i3 = (int)(g / ((long long)l.n_crota * l.n_cdelt2));
    p.d[0] = l.crval1[p.i1];
    p.d[1] = l.crval2[p.i2];
    p.d[2] = l.cdelt1[p.i3];
    p.d[3] = l.cdelt2[p.i4];
    p.d[4] = l.crota[p.i5];
    return p;
}
// _shift_header (alignment.py:401-468) leaves a header: `reference` semantics die on a CDELT2 lag, and a CDELT that a lag
// cancels is no header
bool shiftable(const coreg_wcs2d& small, const LagPoint& p, int sem) {
    if (sem != COREG_CDELT_INTENDED) return p.d[3] == 0.0;
    return small.cdelt1 + p.d[2] != 0.0 && small.cdelt2 + p.d[3] != 0.0;
}
// the lag-point's shifted header, by geometry.hpp (the planners build theirs in two steps)
coreg_wcs2d shifted_header(const coreg_wcs2d& small, const LagPoint& p, int sem) {
    coreg_wcs2d out;
    shift_header(small, p.d[0], p.d[1], p.d[2], p.d[3], p.d[4], sem, &out);
    return out;
}

int params_per_slot(int mode) { return mode == MODE_TRANSLATE ? 2 : 9; }
// parameter k of slot s (of the launch) of launch L
double param(const SweepPlan& sp, const PlannedLaunch& L, int k, size_t s) {
    const size_t ns = (size_t)L.n_batches * 256;
    return sp.params[(size_t)params_per_slot(L.mode) * L.slot_off + (size_t)k * ns + s];
}

// ---- slot coverage ------------------------------------------------------------------------------------------------------
void check_coverage(const char* name, const SweepPlan& sp, const SweepCall& call, const coreg_wcs2d& small) {
    CHECK(!sp.error, "%s: %s", name, sp.error);
    size_t next = 0, n_params = 0;
    for (size_t k = 0; k < sp.launches.size(); ++k) {
        const PlannedLaunch& L = sp.launches[k];
        CHECK(L.slot_off == next, "%s: launch %zu begins at slot %zu, not %zu", name, k, L.slot_off, next);
        CHECK(L.n_batches >= 1, "%s: launch %zu has %d batches", name, k, L.n_batches);
        CHECK(L.n_groups >= 8 && L.n_groups % 8 == 0, "%s: launch %zu has %d groups", name, k, L.n_groups);
        next += (size_t)L.n_batches * 256;
        n_params += (size_t)L.n_batches * 256 * params_per_slot(L.mode);
    }
    CHECK(next == sp.outidx.size(), "%s: the launches hold %zu slots, outidx %zu", name, next, sp.outidx.size());
    CHECK(n_params == sp.params.size(), "%s: the launches hold %zu parameters, params %zu", name, n_params, sp.params.size());
    std::map<long long, int> seen;
    for (long long v : sp.outidx) {
        CHECK(v >= -1, "%s: outidx entry %lld", name, v);
        if (v >= 0) ++seen[v];
    }
    long long expected = 0;
    for (long long idx = call.lag_begin; idx < call.lag_end; ++idx) {
        const bool want = shiftable(small, lag_point(call, idx), call.sem);
        const int got = seen.count(idx) ? seen[idx] : 0;
        CHECK(got == (want ? 1 : 0), "%s: lag index %lld appears %d times, expected %d", name, idx, got, want ? 1 : 0);
        expected += want ? 1 : 0;
    }
    long long live = 0;
    for (auto& kv : seen) {
        CHECK(kv.first >= call.lag_begin && kv.first < call.lag_end, "%s: lag index %lld is outside the slice", name, kv.first);
        live += kv.second;
    }
    CHECK(live == expected, "%s: %lld live slots, %lld lag-points to sweep", name, live, expected);
    CHECK(sp.empty() == (expected == 0), "%s: %zu launches for %lld lag-points", name, sp.launches.size(), expected);
}

// ---- headers ------------------------------------------------------------------------------------------------------------
coreg_wcs2d tan_header(int nx, int ny) {
    coreg_wcs2d w;
    std::memset(&w, 0, sizeof(w));
    w.naxis1 = nx;
    w.naxis2 = ny;
    w.crpix1 = 0.5 * (nx + 1);
    w.crpix2 = 0.5 * (ny + 1);
    w.crval1 = 120.0;  // arcsec
    w.crval2 = -340.0;
    w.cdelt1 = 4.0;
    w.cdelt2 = 4.0;
    w.pc1_1 = w.pc2_2 = 1.0;
    w.unit_to_deg = 1.0 / 3600.0;
    w.lonpole = 180.0;
    w.latpole = kNaN;
    w.dsun_obs = 1.4e11;
    w.crln_obs = 12.0;
    w.crlt_obs = 3.5;
    w.proj = COREG_PROJ_TAN;
    return w;
}
coreg_wcs2d car_header(int nx, int ny) {
    coreg_wcs2d w = tan_header(nx, ny);
    w.crval1 = 30.0;  // degrees
    w.crval2 = 0.0;
    w.cdelt1 = 0.5;
    w.cdelt2 = 0.5;
    w.unit_to_deg = 1.0;
    w.lonpole = kNaN;
    w.proj = COREG_PROJ_CAR;
    return w;
}

// ---- Carrington ---------------------------------------------------------------------------------------------------------
const coreg_carr_grid kGrid = {-20.0, 20.0, 40, -12.0, 12.0, 24, nullptr, nullptr};
const double kSolarR = 1.004;

SweepPlan carrington(const coreg_wcs2d& small, const SweepCall& call, Bench* b) {
    update_carr_tables(b->tabs, b->tabs_key, kGrid, small.crln_obs, nullptr, false);
    return plan_carrington(call, small, kGrid, kSolarR, b->env);
}

void check_carrington(const char* name, const Lags& l, long long begin, long long end, long long c0, long long nc) {
    coreg_wcs2d small = tan_header(32, 24);
    small.cdelt1 = small.cdelt2 = 60.0;
    small.crota = 2.0;
    Bench b(32, 24, kGrid.n_lon, kGrid.n_lat);
    const SweepCall call = make_call(l, begin, end, c0, nc, 2, COREG_CDELT_INTENDED);
    const SweepPlan sp = carrington(small, call, &b);
    check_coverage(name, sp, call, small);
    for (size_t k = 0; k < sp.launches.size(); ++k) {
        const PlannedLaunch& L = sp.launches[k];
        CHECK(L.mode == MODE_TRANSLATE && L.precompute && !L.scan && !L.border_items, "%s: launch %zu is no translation launch", name, k);
        double x0min = 1e300, x0max = -1e300, y0min = 1e300, y0max = -1e300;
        long long first_live = -1;
        for (size_t s = 0; s < (size_t)L.n_batches * 256; ++s) {
            const long long idx = sp.outidx[L.slot_off + s];
            const double x0 = param(sp, L, 0, s), y0 = param(sp, L, 1, s);
            if (idx < 0) {
                CHECK(x0 != x0 && y0 != y0, "%s: padding slot %zu of launch %zu is (%g, %g)", name, s, k, x0, y0);
                continue;
            }
            if (first_live < 0) first_live = idx;
            CHECK(idx % call.d.nc == first_live % call.d.nc, "%s: launch %zu mixes combinations", name, k);
            // utils/rectify.py:396-404 for the shifted header (alignment.py:404-445: CRVAL + lag, CDELT + lag, CROTA + lag)
            const LagPoint p = lag_point(call, idx);
            const double roll = (small.crota + p.d[4]) * (3.14159265358979323846 / 180.0);
            const double v1 = small.crval1 + p.d[0], v2 = small.crval2 + p.d[1];
            const double wx = (small.crpix1 - 1) - (std::cos(roll) * v1 + std::sin(roll) * v2) / (small.cdelt1 + p.d[2]);
            const double wy = (small.crpix2 - 1) - (-std::sin(roll) * v1 + std::cos(roll) * v2) / (small.cdelt2 + p.d[3]);
            // (a handful of roundings on values below 1e4 px)
            CHECK(std::fabs(x0 - wx) <= 1e-11 && std::fabs(y0 - wy) <= 1e-11, "%s: lag %lld has (X0, Y0) = (%.17g, %.17g), rectify gives (%.17g, %.17g)",
                  name, idx, x0, y0, wx, wy);
            x0min = std::min(x0min, x0);
            x0max = std::max(x0max, x0);
            y0min = std::min(y0min, y0);
            y0max = std::max(y0max, y0);
        }
        CHECK(L.f0lo == -x0max && L.f0hi == (double)(b.env.sW - 1) - x0min && L.f1lo == -y0max && L.f1hi == (double)(b.env.sH - 1) - y0min,
              "%s: cull box of launch %zu is (%.17g, %.17g, %.17g, %.17g)", name, k, L.f0lo, L.f0hi, L.f1lo, L.f1hi);
    }
}

// ---- CAR to CAR -----------------------------------------------------------------------------------------------------------
bool fields_equal(const coreg_wcs2d& a, const coreg_wcs2d& b) {
    auto eq = [](double x, double y) { return x == y || (x != x && y != y); };
    const double fa[] = {a.crpix1, a.crpix2, a.crval1, a.crval2, a.cdelt1, a.cdelt2, a.pc1_1, a.pc1_2, a.pc2_1, a.pc2_2, a.unit_to_deg, a.lonpole, a.latpole};
    const double fb[] = {b.crpix1, b.crpix2, b.crval1, b.crval2, b.cdelt1, b.cdelt2, b.pc1_1, b.pc1_2, b.pc2_1, b.pc2_2, b.unit_to_deg, b.lonpole, b.latpole};
    for (size_t k = 0; k < sizeof(fa) / sizeof(fa[0]); ++k)
        if (!eq(fa[k], fb[k])) return false;
    return a.proj == b.proj && a.naxis1 == b.naxis1 && a.naxis2 == b.naxis2;
}

// every rule of the CAR sweep on one request; `want_identity`: lag indices of which the FIRST (in slot order) is to leave
// its launch when the three conditions hold
void check_car(const char* name, const coreg_wcs2d& target, const coreg_wcs2d& small, const Lags& l, Bench* b, int order,
               long long begin = 0, long long end = -1, long long c0 = 0, long long nc = 0) {
    const SweepCall call = make_call(l, begin, end, c0, nc, order, COREG_CDELT_INTENDED);
    const SweepPlan sp = plan_car(call, target, small, b->env);
    check_coverage(name, sp, call, small);
    if (sp.empty()) return;
    const bool same_shape = b->env.gW == b->env.sW && b->env.gH == b->env.sH;
    // the lag-points whose shifted header is the target's
    std::vector<long long> identities;
    for (long long idx = call.lag_begin; idx < call.lag_end; ++idx) {
        const LagPoint p = lag_point(call, idx);
        if (shiftable(small, p, call.sem) && fields_equal(shifted_header(small, p, call.sem), target)) identities.push_back(idx);
    }
    if (std::strstr(name, "identity") && !std::strstr(name, "outside")) CHECK(!identities.empty(), "%s: no identity lag-point in the request", name);
    const bool want_out = b->env.border_fix && same_shape && !identities.empty();
    int n_identity_launches = 0;
    long long taken = -1;
    for (size_t k = 0; k < sp.launches.size(); ++k) {
        const PlannedLaunch& L = sp.launches[k];
        if (L.mode == MODE_CAR) continue;
        ++n_identity_launches;
        CHECK(L.mode == MODE_HOMOGRAPHY && L.n_batches == 1 && L.precompute && L.border_items && !L.scan && k + 1 == sp.launches.size(),
              "%s: launch %zu is no identity launch", name, k);
        taken = sp.outidx[L.slot_off];
        const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int q = 0; q < 9; ++q) CHECK(param(sp, L, q, 0) == ident[q], "%s: identity map element %d is %g", name, q, param(sp, L, q, 0));
        for (size_t s = 1; s < 256; ++s) {
            CHECK(sp.outidx[L.slot_off + s] == -1, "%s: identity launch slot %zu is live", name, s);
            for (int q = 0; q < 9; ++q) CHECK(param(sp, L, q, s) != param(sp, L, q, s), "%s: identity launch padding slot %zu is not NaN", name, s);
        }
        const double inf = std::numeric_limits<double>::infinity();
        CHECK(L.f0lo == -inf && L.f1lo == -inf && L.f0hi == inf && L.f1hi == inf && L.car_fwd.m00 == 0.0 && L.car_fwd.b0 == 0.0,
              "%s: the identity launch culls by position or maps its base coordinates", name);
    }
    CHECK(n_identity_launches == (want_out ? 1 : 0), "%s: %d identity launches, expected %d", name, n_identity_launches, want_out ? 1 : 0);
    if (want_out) {
        bool is_one = false;
        for (long long v : identities) is_one = is_one || v == taken;
        CHECK(is_one, "%s: lag %lld was taken out and is no identity lag-point", name, taken);
        CHECK((order & 1) ? (sp.fix.items.size() == 1 && sp.flags.size() == 1 && sp.flags[0].size() == (size_t)b->env.gW * b->env.gH)
                          : (sp.flags.empty() && sp.fix.items.size() == (sp.fix.pixels.empty() ? 0u : 1u)),
              "%s: the identity launch carries %zu items and %zu flag grids", name, sp.fix.items.size(), sp.flags.size());
    }
    // the CAR launches: parameters, skip bytes, pole_sep
    Mat3 r_target;
    CHECK(car_native_to_celestial(target, &r_target) == 0, "%s: the target header has no native pole", name);
    bool redo_expected = true;
    int last_groups = -1, last_batches = -1, n_invalid = 0;
    for (size_t k = 0; k < sp.launches.size(); ++k) {
        const PlannedLaunch& L = sp.launches[k];
        if (L.mode != MODE_CAR) continue;
        // k_tile_list is redone only when the groups or the batches change
        redo_expected = L.n_groups != last_groups || L.n_batches != last_batches;
        CHECK(L.precompute == redo_expected, "%s: launch %zu %s its precompute", name, k, L.precompute ? "runs" : "skips");
        last_groups = L.n_groups;
        last_batches = L.n_batches;
        const size_t ns = (size_t)L.n_batches * 256;
        CHECK(L.tap_skip.size() == ns && L.i1.size() == ns && L.i2.size() == ns && L.hc.size() == 1 && !L.border_items,
              "%s: launch %zu lists %zu skip bytes for %zu slots", name, k, L.tap_skip.size(), ns);
        if (L.tap_skip.size() != ns) continue;
        double pole_sep = 0.0;
        bool any_scan = false;
        for (size_t s = 0; s < ns; ++s) {
            const long long idx = sp.outidx[L.slot_off + s];
            bool valid = false, on_axis = false;
            if (idx >= 0) {
                const LagPoint p = lag_point(call, idx);
                const coreg_wcs2d hl = shifted_header(small, p, call.sem);
                Mat3 rs;
                valid = car_native_to_celestial(hl, &rs) == 0;
                n_invalid += valid ? 0 : 1;
                on_axis = hl.crval1 == target.crval1 || hl.crval2 == target.crval2;
                const double r8 = param(sp, L, 8, s);
                if (valid) {
                    // R = R_shifted^T R_target; long double products, so 1e-15 covers the rounding to double
                    const Mat3 m = mat_mul(mat_T(rs), r_target);
                    for (int q = 0; q < 9; ++q)
                        CHECK(std::fabs(param(sp, L, q, s) - (double)m.m[q / 3][q % 3]) <= 1e-15, "%s: lag %lld rotation element %d", name, idx, q);
                    pole_sep = std::max(pole_sep, std::acos(std::fmax(-1.0, std::fmin(1.0, r8))));
                    const coreg_wcs2d scan = sp.shifted_of(L, *call.lags, (int)s);
                    CHECK(fields_equal(scan, hl), "%s: the scan's header of lag %lld is not its shifted header", name, idx);
                } else {
                    for (int q = 0; q < 9; ++q) CHECK(param(sp, L, q, s) != param(sp, L, q, s), "%s: lag %lld has no native pole and parameter %d is %g", name, idx, q, param(sp, L, q, s));
                }
            } else {
                for (int q = 0; q < 9; ++q) CHECK(param(sp, L, q, s) != param(sp, L, q, s), "%s: padding slot %zu of launch %zu is not NaN", name, s, k);
            }
            const bool scanned = idx >= 0 && valid && b->env.tap_fix && same_shape && on_axis;
            CHECK(L.tap_skip[s] == (scanned ? 0 : 1), "%s: slot %zu of launch %zu (lag %lld) has skip byte %d", name, s, k, idx, (int)L.tap_skip[s]);
            any_scan = any_scan || scanned;
        }
        CHECK(L.scan == any_scan, "%s: launch %zu %s", name, k, L.scan ? "scans" : "does not scan");
        CHECK(L.car_inv.pole_sep == pole_sep, "%s: launch %zu has pole_sep %.17g, its valid lags give %.17g", name, k, L.car_inv.pole_sep, pole_sep);
    }
    if (std::strstr(name, "poles")) CHECK(n_invalid > 0, "%s: every lag has a native pole", name);
}

void car_rules() {
    const coreg_wcs2d hdr = car_header(32, 24);
    Lags l({-1.0, 0.0, 1.0}, {-0.5, 0.0, 0.5}, {0.0, 0.01}, {0.0}, {0.0, 0.2});
    for (int order = 1; order <= 3; ++order) {
        Bench b(32, 24, 32, 24);
        check_car("car identity", hdr, hdr, l, &b, order);
    }
    {
        Bench b(32, 24, 32, 24);
        b.env.border_fix = false;
        check_car("car identity, border_fix off", hdr, hdr, l, &b, 3);
    }
    {
        Bench b(30, 24, 32, 24);  // (another image shape)
        check_car("car identity, shapes differ", hdr, hdr, l, &b, 3);
    }
    {
        Bench b(32, 24, 32, 24);
        coreg_wcs2d target = hdr;
        target.crpix1 += 0.5;
        check_car("car, CRPIX1 differs", target, hdr, l, &b, 3);
        target = hdr;
        target.latpole = 90.0;  // (NaN on the other side)
        check_car("car, LATPOLE differs", target, hdr, l, &b, 3);
    }
    {
        Bench b(32, 24, 32, 24);
        b.env.tap_fix = false;
        check_car("car identity, tap_fix off", hdr, hdr, l, &b, 3);
    }
    {
        Bench b(32, 24, 32, 24);
        Lags twice({0.0, 1.0, 0.0}, {0.0, 0.5}, {0.0}, {0.0}, {0.0});
        check_car("car, two identity lag-points", hdr, hdr, twice, &b, 3);
        check_car("car identity outside the slice", hdr, hdr, twice, &b, 3, 1, 2);
    }
    {
        // an explicit LONPOLE of 90 degrees leaves a native pole only to the maps whose CRVAL2 is 0
        Bench b(32, 24, 32, 24);
        coreg_wcs2d h90 = hdr;
        h90.lonpole = 90.0;
        Lags poles({-1.0, 0.0, 1.0}, {0.0, 0.5, -0.5, 1.0}, {0.0}, {0.0}, {0.0, 0.2});
        check_car("car poles", h90, h90, poles, &b, 2);
    }
    {
        Bench b(32, 24, 32, 24);
        coreg_wcs2d bad = hdr;
        bad.lonpole = 90.0;
        bad.crval2 = 10.0;
        Lags one({0.0}, {0.0}, {0.0}, {0.0}, {0.0});
        const SweepPlan sp = plan_car(make_call(one, 0, -1, 0, 0, 2, COREG_CDELT_INTENDED), bad, hdr, b.env);
        CHECK(sp.error && sp.empty(), "car: a target header without a native pole is planned");
    }
}

// ---- TAN ------------------------------------------------------------------------------------------------------------------
// eps_max as the kernels' series form needs it bounded: the largest |h6| gW + |h7| gH over the lags
double eps_max_of(const SweepCall& call, const coreg_wcs2d& target, const coreg_wcs2d& small, const Bench& b) {
    double e = 0.0;
    for (long long idx = call.lag_begin; idx < call.lag_end; ++idx) {
        const LagPoint p = lag_point(call, idx);
        if (!shiftable(small, p, call.sem)) continue;
        double hm[9];
        homography(target, shifted_header(small, p, call.sem), hm);
        e = std::max(e, std::fabs(hm[6]) * b.env.gW + std::fabs(hm[7]) * b.env.gH);
    }
    return e;
}

// rows / columns of the grid that the lag-point's map leaves where they are, by the lag alone (the headers are unrotated):
// on the target's tangent point with no CROTA lag, a CDELT1 lag stretches x only and a CDELT2 lag y only
void invariant_axes(const coreg_wcs2d& target, const coreg_wcs2d& hl, const LagPoint& p, bool* rows, bool* cols) {
    const bool on_tangent = hl.crval1 == target.crval1 && hl.crval2 == target.crval2 && p.d[4] == 0.0;
    *rows = on_tangent && p.d[3] == 0.0;
    *cols = on_tangent && p.d[2] == 0.0;
}

void check_tan(const char* name, const coreg_wcs2d& target, const coreg_wcs2d& small, const Lags& l, Bench* b, int order,
               long long begin = 0, long long end = -1, long long c0 = 0, long long nc = 0, int sem = COREG_CDELT_INTENDED) {
    const SweepCall call = make_call(l, begin, end, c0, nc, order, sem);
    const SweepPlan sp = plan_tan(call, target, small, b->env);
    check_coverage(name, sp, call, small);
    if (sp.empty()) return;
    CHECK(sp.launches.size() == 1, "%s: %zu launches", name, sp.launches.size());
    const PlannedLaunch& L = sp.launches[0];
    const size_t ns = sp.outidx.size();
    CHECK(L.precompute && L.border_items && L.scan == b->env.tap_fix, "%s: the launch's flags", name);
    const double eps = eps_max_of(call, target, small, *b);
    const int want_mode = (b->env.h_series && eps < 4.0e-6) ? MODE_HOMOGRAPHY_SERIES : MODE_HOMOGRAPHY;
    CHECK(L.mode == want_mode, "%s: sweep mode %d for eps_max %.3g", name, L.mode, eps);
    if (b->env.tap_fix) CHECK(L.tap_skip.size() == ns && L.i1.size() == ns && L.slot_hc.size() == ns, "%s: %zu skip bytes for %zu slots", name, L.tap_skip.size(), ns);
    const double gx[5] = {0.0, (double)(b->env.gW - 1), 0.0, (double)(b->env.gW - 1), 0.5 * (b->env.gW - 1)};
    const double gy[5] = {0.0, 0.0, (double)(b->env.gH - 1), (double)(b->env.gH - 1), 0.5 * (b->env.gH - 1)};
    size_t n_items = 0, n_flags = 0;
    for (size_t s = 0; s < ns; ++s) {
        const long long idx = sp.outidx[s];
        if (idx < 0) {
            for (int q = 0; q < 9; ++q) CHECK(param(sp, L, q, s) != param(sp, L, q, s), "%s: padding slot %zu is not NaN", name, s);
            if (b->env.tap_fix && L.tap_skip.size() == ns) CHECK(L.tap_skip[s] == 1, "%s: padding slot %zu is scanned", name, s);
            continue;
        }
        const LagPoint p = lag_point(call, idx);
        const coreg_wcs2d hl = shifted_header(small, p, call.sem);
        double want[9], got[9];
        homography(target, hl, want);
        for (int q = 0; q < 9; ++q) got[q] = param(sp, L, q, s);
        for (int c = 0; c < 5; ++c) {
            double x0, y0, x1, y1;
            apply_h(want, gx[c], gy[c], &x0, &y0);
            apply_h(got, gx[c], gy[c], &x1, &y1);
            CHECK(std::fabs(x0 - x1) <= 1e-6 && std::fabs(y0 - y1) <= 1e-6, "%s: lag %lld maps (%g, %g) to (%.9f, %.9f), homography() to (%.9f, %.9f)",
                  name, idx, gx[c], gy[c], x1, y1, x0, y0);
            // every cull box holds what can be in bounds
            if (x1 >= 0.0 && x1 <= b->env.sW - 1 && y1 >= 0.0 && y1 <= b->env.sH - 1)
                CHECK(gx[c] >= L.f0lo && gx[c] <= L.f0hi && gy[c] >= L.f1lo && gy[c] <= L.f1hi, "%s: the cull box drops (%g, %g), in bounds for lag %lld", name, gx[c], gy[c], idx);
        }
        if (b->env.tap_fix && L.tap_skip.size() == ns)
            CHECK(fields_equal(sp.shifted_of(L, *call.lags, (int)s), hl), "%s: the scan's header of lag %lld is not its shifted header", name, idx);
        bool rows, cols;
        invariant_axes(target, hl, p, &rows, &cols);
        const bool noise_decided = b->env.border_fix && (rows || cols);
        if (b->env.tap_fix && L.tap_skip.size() == ns)
            CHECK(L.tap_skip[s] == (noise_decided ? 1 : 0), "%s: lag %lld has skip byte %d", name, idx, (int)L.tap_skip[s]);
        const BorderItems::Item* item = nullptr;
        for (const BorderItems::Item& it : sp.fix.items)
            if (it.slot == (long long)s) item = &it;
        if (!noise_decided) {
            CHECK(!item, "%s: lag %lld carries a BorderFix item", name, idx);
            continue;
        }
        // the pixels of the invariant border rows / columns that wcslib's round trip sends out of the image, row-major
        WcslibTan wf, wt;
        wf.init(target);
        wt.init(hl);
        std::vector<int> dropped;
        for (int j = 0; j < b->env.gH; ++j)
            for (int i = 0; i < b->env.gW; ++i) {
                const bool on_row = rows && (j == 0 || j == b->env.sH - 1), on_col = cols && (i == 0 || i == b->env.sW - 1);
                if (!on_row && !on_col) continue;
                double x, y;
                wcslib_pixel_to_pixel(wf, wt, (double)i, (double)j, &x, &y);
                if (!(x >= 0.0 && x <= b->env.sW - 1 && y >= 0.0 && y <= b->env.sH - 1)) dropped.push_back(j * b->env.gW + i);
            }
        const bool want_item = (order & 1) || !dropped.empty();
        CHECK((item != nullptr) == want_item, "%s: lag %lld %s a BorderFix item (%zu pixels dropped)", name, idx, item ? "carries" : "lacks", dropped.size());
        if (!item) continue;
        ++n_items;
        CHECK(item->first >= 0 && item->n >= 0 && (size_t)(item->first + item->n) <= sp.fix.pixels.size() && (size_t)item->n == dropped.size() &&
                  std::equal(dropped.begin(), dropped.end(), sp.fix.pixels.begin() + item->first),
              "%s: lag %lld lists %d dropped pixels, the border loop finds %zu", name, idx, item->n, dropped.size());
        if (order & 1) {
            const size_t each = (size_t)b->env.gW * b->env.gH;
            CHECK(item->flags_off >= 0 && item->flags_off % (long long)each == 0 && (size_t)(item->flags_off / (long long)each) < sp.flags.size(),
                  "%s: lag %lld has flags offset %lld", name, idx, item->flags_off);
            ++n_flags;
        } else {
            CHECK(item->flags_off == -1, "%s: lag %lld has flags at an even order", name, idx);
        }
        // the snapped map is exactly invariant along the axis
        if (rows) CHECK(got[3] == 0.0 && got[4] == 1.0 && got[5] == 0.0 && got[6] == 0.0 && got[7] == 0.0, "%s: lag %lld: rows are not mapped to themselves exactly", name, idx);
        if (cols) CHECK(got[0] == 1.0 && got[1] == 0.0 && got[2] == 0.0 && got[6] == 0.0 && got[7] == 0.0, "%s: lag %lld: columns are not mapped to themselves exactly", name, idx);
    }
    CHECK(sp.fix.items.size() == n_items && sp.flags.size() == n_flags, "%s: %zu items and %zu flag grids, %zu and %zu expected", name,
          sp.fix.items.size(), sp.flags.size(), n_items, n_flags);
    if (std::strstr(name, "sub-map") && b->env.border_fix && (order & 1)) CHECK(n_items == 3,"%s: %zu noise-decided lag-points in the request", name, n_items);
    for (const auto& f : sp.flags) CHECK(f.size() == (size_t)b->env.gW * b->env.gH, "%s: a flag grid of %zu entries", name, f.size());
}

void tan_rules() {
    const coreg_wcs2d hdr = tan_header(32, 24);
    // zero CRVAL lags (the tangent point of the target) with and without CDELT / CROTA lags on top
    Lags l({-8.0, 0.0, 8.0, 16.0}, {0.0, -8.0, 8.0}, {0.0, 0.05}, {0.0, -0.05}, {0.0, 0.3});
    for (int order = 2; order <= 3; ++order) {
        Bench b(32, 24, 32, 24);
        check_tan("tan sub-map", hdr, hdr, l, &b, order);
        Bench b2(32, 24, 32, 24);
        b2.env.tap_fix = false;
        check_tan("tan sub-map, tap_fix off", hdr, hdr, l, &b2, order);
        Bench b3(32, 24, 32, 24);
        b3.env.border_fix = false;
        check_tan("tan sub-map, border_fix off", hdr, hdr, l, &b3, order);
    }
    {
        // a larger target grid around the image to align: no lag-point on its tangent point
        coreg_wcs2d target = tan_header(48, 32);
        target.crval1 += 3.0;
        Bench b(32, 24, 48, 32);
        check_tan("tan wide grid", target, hdr, l, &b, 3);
        check_tan("tan wide grid, reference CDELT semantics", target, hdr, l, &b, 2, 0, -1, 0, 0, COREG_CDELT_REFERENCE);
    }
    {
        // the series form: eps_max a factor of 10 below and above 4e-6 (eps ~ tan(lag) x 32 px x 4 arcsec)
        Bench b(32, 24, 32, 24);
        Lags near({-60.0, 0.0, 60.0}, {-50.0, 50.0}, {0.0}, {0.0}, {0.0});
        Lags far({-13000.0, 0.0, 13000.0}, {-10000.0, 10000.0}, {0.0}, {0.0}, {0.0});
        const double e_near = eps_max_of(make_call(near, 0, -1, 0, 0, 2, COREG_CDELT_INTENDED), hdr, hdr, b);
        const double e_far = eps_max_of(make_call(far, 0, -1, 0, 0, 2, COREG_CDELT_INTENDED), hdr, hdr, b);
        CHECK(e_near < 4.0e-7 && e_near > 4.0e-8, "tan: eps_max of the near lag set is %.3g", e_near);
        CHECK(e_far > 4.0e-5 && e_far < 4.0e-4, "tan: eps_max of the far lag set is %.3g", e_far);
        check_tan("tan near lags", hdr, hdr, near, &b, 2);
        check_tan("tan far lags", hdr, hdr, far, &b, 2);
        b.env.h_series = false;
        check_tan("tan near lags, h_series off", hdr, hdr, near, &b, 2);
    }
}

// ---- slot coverage over the slices, combination ranges and lag orders -------------------------------------------------------
void coverage_rules() {
    struct Case {
        const char* name;
        long long begin, end, c0, nc;
    };
    // 5 x 4 x 2 x 1 x 2 lags: 4 combinations, 16 lag indices per CRVAL1 value, 80 in all
    const Case cases[] = {{"whole", 0, -1, 0, 0},           {"mid-row slice", 7, 75, 0, 0},     {"one lag-point", 9, 10, 0, 0},
                          {"one row, mid to mid", 18, 29, 0, 0}, {"empty slice", 5, 5, 0, 0},   {"one combination of four", 0, -1, 2, 1},
                          {"two combinations, mid-row", 3, 33, 1, 2}};
    const std::vector<double> a1[] = {{-2.0, -1.0, 0.0, 1.0, 2.0}, {2.0, 1.0, 0.0, -1.0, -2.0}, {1.0, -2.0, 2.0, 0.0, -1.0}};
    const std::vector<double> a2[] = {{-1.5, -0.5, 0.5, 1.5}, {1.5, 0.5, -0.5, -1.5}, {0.5, -1.5, 1.5, -0.5}};
    const char* orders[] = {"ascending", "descending", "shuffled"};
    for (int o = 0; o < 3; ++o)
        for (const Case& c : cases) {
            const std::string name = std::string(c.name) + ", " + orders[o];
            {   // Carrington: lags in arcsec
                std::vector<double> s1 = a1[o], s2 = a2[o];
                for (double& v : s1) v *= 30.0;
                for (double& v : s2) v *= 30.0;
                Lags l(s1, s2, {0.0, 0.5}, {0.0}, {0.0, 0.4});
                check_carrington(("carrington " + name).c_str(), l, c.begin, c.end, c.c0, c.nc);
            }
            {   // CAR: degrees, the identity lag-point among them
                Lags l(a1[o], a2[o], {0.0, 0.01}, {0.0}, {0.0, 0.2});
                Bench b(32, 24, 32, 24);
                const coreg_wcs2d hdr = car_header(32, 24);
                check_car(("car " + name).c_str(), hdr, hdr, l, &b, 3, c.begin, c.end, c.c0, c.nc);
            }
            {   // TAN: arcsec, the zero lag among them
                std::vector<double> s1 = a1[o], s2 = a2[o];
                for (double& v : s1) v *= 6.0;
                for (double& v : s2) v *= 6.0;
                s2[o == 0 ? 1 : (o == 1 ? 2 : 3)] = 0.0;  // (-0.5 -> 0: a zero CRVAL2 lag)
                Lags l(s1, s2, {0.0, 0.05}, {0.0}, {0.0, 0.3});
                Bench b(32, 24, 32, 24);
                const coreg_wcs2d hdr = tan_header(32, 24);
                check_tan(("tan " + name).c_str(), hdr, hdr, l, &b, 3, c.begin, c.end, c.c0, c.nc);
            }
        }
    {
        // a CDELT1 lag that cancels CDELT1 leaves no header: its combinations stay NaN
        Lags l({-30.0, 0.0, 30.0}, {0.0, 30.0}, {0.0, -60.0}, {0.0}, {0.0, 0.4});
        check_carrington("carrington, a CDELT1 lag cancels CDELT1", l, 0, -1, 0, 0);
        Lags lt({-6.0, 0.0, 6.0}, {0.0, 6.0}, {0.0, -4.0}, {0.0}, {0.0});
        Bench b(32, 24, 32, 24);
        const coreg_wcs2d hdr = tan_header(32, 24);
        check_tan("tan, a CDELT1 lag cancels CDELT1", hdr, hdr, lt, &b, 2);
        // `reference` semantics: every CDELT2 lag kills the worker -- nothing to launch
        Lags l2({-6.0, 0.0}, {0.0}, {0.0}, {0.1}, {0.0});
        check_tan("tan, reference semantics with a CDELT2 lag", hdr, hdr, l2, &b, 2, 0, -1, 0, 0, COREG_CDELT_REFERENCE);
    }
    {
        // more than one batch per combination: 20 x 16 lags of one combination
        std::vector<double> s1, s2;
        for (int i = 0; i < 20; ++i) s1.push_back(3.0 * (i - 10));
        for (int i = 0; i < 16; ++i) s2.push_back(3.0 * (i - 8));
        Lags l(s1, s2, {0.0}, {0.0}, {0.0});
        check_carrington("carrington 20 x 16", l, 5, 311, 0, 0);
        Bench b(32, 24, 32, 24);
        const coreg_wcs2d hdr = tan_header(32, 24);
        check_tan("tan 20 x 16", hdr, hdr, l, &b, 2, 5, 311);
    }
}

// ---- determinism ------------------------------------------------------------------------------------------------------------
bool same_bytes(const SweepPlan& a, const SweepPlan& b) {
    return a.params.size() == b.params.size() && a.outidx.size() == b.outidx.size() &&
           std::memcmp(a.params.data(), b.params.data(), a.params.size() * sizeof(double)) == 0 &&
           std::memcmp(a.outidx.data(), b.outidx.data(), a.outidx.size() * sizeof(long long)) == 0;
}

void determinism() {
    Lags l({-8.0, 0.0, 8.0, 16.0, 24.0}, {0.0, -8.0, 8.0, 4.0}, {0.0, 0.05}, {0.0}, {0.0, 0.3});
    const coreg_wcs2d hdr = tan_header(32, 24);
    const SweepCall call = make_call(l, 7, 75, 0, 0, 3, COREG_CDELT_INTENDED);
    Bench b(32, 24, 32, 24);
    const SweepPlan first = plan_tan(call, hdr, hdr, b.env);
    CHECK(!first.empty(), "determinism: nothing planned");
    CHECK(same_bytes(first, plan_tan(call, hdr, hdr, b.env)), "tan: planning twice differs");  // (memo and caches warm)
    for (unsigned nt : {1u, 8u}) {
        Bench c(32, 24, 32, 24);
        c.env.plan_threads = nt;
        CHECK(same_bytes(first, plan_tan(call, hdr, hdr, c.env)), "tan: planning on %u threads differs", nt);
    }
    const coreg_wcs2d car = car_header(32, 24);
    Lags lc({-1.0, 0.0, 1.0}, {-0.5, 0.0, 0.5}, {0.0, 0.01}, {0.0}, {0.0, 0.2});
    const SweepCall cc = make_call(lc, 3, 30, 0, 0, 3, COREG_CDELT_INTENDED);
    const SweepPlan car1 = plan_car(cc, car, car, b.env);
    CHECK(!car1.empty() && same_bytes(car1, plan_car(cc, car, car, b.env)), "car: planning twice differs");
    coreg_wcs2d small = tan_header(32, 24);
    small.cdelt1 = small.cdelt2 = 60.0;
    Bench g(32, 24, kGrid.n_lon, kGrid.n_lat);
    Lags lg({-60.0, 0.0, 60.0}, {-30.0, 30.0}, {0.0, 0.5}, {0.0}, {0.0, 0.4});
    const SweepCall cg = make_call(lg, 1, 20, 0, 0, 2, COREG_CDELT_INTENDED);
    const SweepPlan g1 = carrington(small, cg, &g);
    CHECK(!g1.empty() && same_bytes(g1, carrington(small, cg, &g)), "carrington: planning twice differs");
}

// ---- the single-sample lists ----------------------------------------------------------------------------------------------------
// Whatever order the scan listed the samples in: one segment per listed slot, slots ascending, a segment's pixels ascending,
// every sample once, and the coordinates those of wcslib's round trip under the slot's header.
void tap_lists(bool car) {
    const char* name = car ? "tap lists (CAR)" : "tap lists (TAN)";
    const coreg_wcs2d hdr = car ? car_header(32, 24) : tan_header(32, 24);
    const int gw = 32, n_slots = 12;
    auto shifted_of = [&](int slot) {
        coreg_wcs2d hl = hdr;
        hl.crval1 += (car ? 0.01 : 3.0) * slot;
        return hl;
    };
    std::vector<TapSample> list;
    std::map<unsigned, std::vector<unsigned>> want;
    uint32_t s = 99u;
    for (int k = 0; k < 300; ++k) {
        s = s * 1664525u + 1013904223u;
        const unsigned slot = (s >> 8) % 5u * 2u + 1u;  // (slots 1, 3, .. 9 only: the others list nothing)
        const unsigned pixel = (unsigned)k * 7u % (32u * 24u);
        list.push_back({slot, pixel});
        want[slot].push_back(pixel);
    }
    const TapLists t = group_tap_samples(list, n_slots, gw, hdr, shifted_of);
    CHECK(t.seg_slot.size() == want.size() && t.seg_begin.size() == want.size() + 1 && t.pixel.size() == list.size() &&
              t.xw.size() == list.size() && t.yw.size() == list.size(), "%s: %zu segments, %zu entries", name, t.seg_slot.size(), t.pixel.size());
    if (t.seg_slot.size() != want.size() || t.seg_begin.size() != want.size() + 1 || t.pixel.size() != list.size()) return;
    CHECK(t.seg_begin.front() == 0 && t.seg_begin.back() == (int)list.size(), "%s: the segments span [%d, %d)", name, t.seg_begin.front(), t.seg_begin.back());
    size_t sg = 0;
    for (auto& kv : want) {
        std::sort(kv.second.begin(), kv.second.end());
        CHECK(t.seg_slot[sg] == (int)kv.first, "%s: segment %zu is slot %d, not %u", name, sg, t.seg_slot[sg], kv.first);
        const int b = t.seg_begin[sg], e = t.seg_begin[sg + 1];
        CHECK(e - b == (int)kv.second.size() && std::equal(kv.second.begin(), kv.second.end(), t.pixel.begin() + b),
              "%s: segment %zu does not hold slot %u's pixels in order", name, sg, kv.first);
        for (int q = b; q < e && e - b == (int)kv.second.size(); ++q) {
            double x, y;
            if (car) {
                WcslibCar wf, wt;
                wf.init(hdr);
                wt.init(shifted_of((int)kv.first));
                wcslib_pixel_to_pixel(wf, wt, (double)(t.pixel[q] % gw), (double)(t.pixel[q] / gw), &x, &y);
            } else {
                WcslibTan wf, wt;
                wf.init(hdr);
                wt.init(shifted_of((int)kv.first));
                wcslib_pixel_to_pixel(wf, wt, (double)(t.pixel[q] % gw), (double)(t.pixel[q] / gw), &x, &y);
            }
            CHECK(t.xw[q] == x && t.yw[q] == y, "%s: entry %d has (%.17g, %.17g), the round trip gives (%.17g, %.17g)", name, q, t.xw[q], t.yw[q], x, y);
        }
        ++sg;
    }
    const TapLists none = group_tap_samples(std::vector<TapSample>(), n_slots, gw, hdr, shifted_of);
    CHECK(none.seg_slot.empty() && none.seg_begin.size() == 1 && none.seg_begin[0] == 0, "%s: an empty list gives %zu segments", name, none.seg_slot.size());
}

// ---- the caches keep their limits ---------------------------------------------------------------------------------------------
void cache_limits() {
    Bench b(32, 24, 32, 24);
    const coreg_wcs2d hdr = tan_header(32, 24);
    AxisInvariance inv;
    inv.rows = inv.cols = true;
    for (int k = 0; k < 70; ++k) {
        coreg_wcs2d hl = hdr;
        hl.cdelt1 += 1e-3 * k;
        std::vector<int> out;
        wcslib_dropped_border_pixels(b.env, hdr, hl, inv, &out);
        CHECK(b.caches.border.size() <= 64 && b.caches.border.size() == (size_t)(k % 64) + 1, "border cache holds %zu entries after %d headers", b.caches.border.size(), k + 1);
        wcslib_tap_shift_flags(b.env, hdr, hl, inv);
        CHECK(b.caches.flags.size() <= 4 && b.caches.flags.size() == (size_t)(k % 4) + 1, "flags cache holds %zu entries after %d headers", b.caches.flags.size(), k + 1);
    }
}
}  // namespace

int main() {
    coverage_rules();
    car_rules();
    tan_rules();
    determinism();
    tap_lists(false);
    tap_lists(true);
    cache_limits();
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: sweep plan rules (%d checks)\n", n_checked);
    return 0;
}
