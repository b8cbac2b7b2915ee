// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): C ABI: coreg_sweep_carrington / coreg_sweep_helioprojective (each launch described by a SweepLaunchSpec),
// grid-shared sums, pivots, stats.
#pragma once
namespace {
// ---- the steps every sweep shares ---------------------------------------------------------------------------------
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

// The checks and set-up of the public sweeps, in this order: method, order, the entry point's own checks (`own_checks`),
// the lag set with the combination range the entry point took off the handle, the device, the reference-on-grid shape
// (`grid_w` x `grid_h`, `grid_what` names it), begin_sweep.  With nothing to sweep (call->n_out == 0) the caller returns
// end_sweep at once.
template <typename OwnChecks>
int open_sweep(coreg_handle* h, ComboRange combo, OwnChecks own_checks, const coreg_lags* lags, int order, int method,
               int sem, int64_t lag_begin, int64_t lag_end, int grid_w, int grid_h, const char* grid_what,
               double* corr_out, int out_on_device, SweepCall* call) {
    if (method != COREG_METHOD_CORRELATION && method != COREG_METHOD_RESIDUS && method != COREG_METHOD_RESIDUS_MASKED)
        return fail(h, COREG_ENOTIMPL,
                    "method must be COREG_METHOD_CORRELATION, COREG_METHOD_RESIDUS or COREG_METHOD_RESIDUS_MASKED");
    RETCHK(check_order(h, order));
    RETCHK(own_checks());
    RETCHK(check_lags(h, lags, &call->d, lag_begin, lag_end, combo));
    RETCHK(bind_device_nowait(h));  // (the image to align is joined right before k_sweep: launch_sweep)
    if (h->ref.p && (h->gW != grid_w || h->gH != grid_h))
        return fail(h, COREG_EINVAL, std::string("reference-on-grid shape differs from ") + grid_what);
    call->lags = lags;
    call->order = order;
    call->method = method;
    call->sem = sem;
    call->lag_begin = lag_begin;
    call->lag_end = lag_end;
    call->n_out = lag_end - lag_begin;
    call->corr_out = corr_out;
    call->out_on_device = out_on_device;
    return begin_sweep(h, call->n_out, corr_out, out_on_device, &call->out_dev);
}

int close_sweep(coreg_handle* h, const SweepCall& call) {
    return end_sweep(h, call.n_out, call.corr_out, call.out_on_device, call.out_dev);
}

// a plan without a launch: every lag-point NaN
int close_empty_sweep(coreg_handle* h, const SweepCall& call) {
    RETCHK(fill_nan(h, call.out_dev, call.n_out));
    RETCHK(fill_nan(h, h->counts.as<double>(), call.n_out));
    return close_sweep(h, call);
}

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
Plan plan_sweep(coreg_handle* h, const Geometry& geo, const SweepCall& call) {
    return choose_plan(h, geo, call.i1_hi() - call.i1_lo() + 1, call.d.n2, h->opt_use_lds ? lds_window_elems(h) : (1LL << 40));
}

// Combination c of the sweep: its (CDELT, CROTA)-shifted header and its lag slots.  False: nothing of it to launch (no
// lag of the slice, or a lag that kills the reference's worker: NaN, already filled).  Pure: called from threads.
bool combo_slots(const SweepCall& call, const coreg_wcs2d& small, const Plan& plan, long long c, coreg_wcs2d* hc,
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

// launch_precompute (unless `launch` is false: the compacted points are still those of the same arguments), and keep how
// to launch it again: a grid-shared sweep's coreg_finalize_sums re-evaluates a launch after later launches have run
template <int MODE>
int precompute(coreg_handle* h, const PrecomputeArgs& pa, int n_tiles, int n_groups, int n_batches, bool launch = true) {
    if (launch) RETCHK(launch_precompute<MODE>(h, pa, n_tiles, n_groups, n_batches));
    h->last_precompute = [pa, n_tiles, n_groups, n_batches](coreg_handle* hh) {
        return launch_precompute<MODE>(hh, pa, n_tiles, n_groups, n_batches);
    };
    return COREG_OK;
}

// The launch of `call` whose slots start at slot `slot_off` of the uploaded plan; the entry point adds what only it has
// (car_inv, fix, pitch_sel).
SweepLaunchSpec sweep_launch(const SweepCall& call, int mode, size_t slot_off, int n_batches, int n_tiles) {
    SweepLaunchSpec sl;
    sl.mode = mode;
    sl.order = call.order;
    sl.method = call.method;
    sl.slot_off = slot_off;
    sl.n_batches = n_batches;
    sl.n_tiles = n_tiles;
    sl.lag_begin = call.lag_begin;
    sl.out_dev = call.out_dev;
    return sl;
}

// k_finalize of pending launch `pf` of a grid-shared sweep, from the reduced sums (work-space pointers taken afresh: a
// later launch of the sweep may have grown the buffers)
int finalize_pending(coreg_handle* h, const coreg_handle::PendingFinalize& pf, long long* refine_count, double* out_dev,
                     FinalizeArgs* f) {
    *f = FinalizeArgs{};
    RETCHK(fill_refine(h, &f->refine, pf.refine.mode, pf.refine.order, pf.refine.lane_params, pf.refine.car_inv,
                       pf.n_slots));
    f->refine.enabled = pf.refine.enabled;
    f->refine_count = refine_count;
    f->partials = h->sums.as<double>() + pf.slot_off;
    f->n_groups = 1;
    f->n_slots = pf.n_slots;
    f->part_stride = h->sums_slots;
    f->out_index = h->fin_outidx.as<long long>() + pf.slot_off;
    f->lag_begin = pf.lag_begin;
    f->out = out_dev;
    f->counts = h->counts.as<double>();
    f->residus = pf.residus;
    f->n_required = (long long)h->gW * h->gH;
    launch_finalize(h, *f);
    return COREG_OK;
}
}  // namespace

extern "C" {
int coreg_sweep_carrington(coreg_handle* h, const coreg_wcs2d* hdr_small, const coreg_carr_grid* grid, double solar_r,
                           const coreg_lags* lags, int order, int method, int cdelt_semantics, int64_t lag_begin,
                           int64_t lag_end, double* corr_out, int out_on_device) {
    if (!h) return COREG_EINVAL;
    const ComboRange combo = take_combo_range(h);
    trace("sweep_carrington: enter");
    if (!hdr_small || !grid) return fail(h, COREG_EINVAL, "sweep_carrington: null header/grid");
    auto own_checks = [&] {
        RETCHK(check_wcs(h, hdr_small, true));
        RETCHK(check_grid(h, grid));
        if (!std::isfinite(solar_r) || !(solar_r > 0.0)) return fail(h, COREG_EINVAL, "solar_r must be positive");
        return COREG_OK;
    };
    SweepCall call;
    RETCHK(open_sweep(h, combo, own_checks, lags, order, method, cdelt_semantics, lag_begin, lag_end, grid->n_lon,
                      grid->n_lat, "the Carrington grid", corr_out, out_on_device, &call));
    if (call.n_out == 0) return close_sweep(h, call);  // (nothing to fill)
    const LagDims& d = call.d;

    CarrDev cd;
    std::memset(&cd, 0, sizeof(cd));
    RETCHK(upload_carr_tables(h, *grid, *hdr_small, &cd, h->has_rot_small ? &h->rot_small : nullptr));
    // differential rotation: neighbouring rows slide against each other by up to this many radians of longitude, which
    // the whole-tile bound below adds to the per-row step
    double row_slip = 0.0;
    for (size_t j = 1; j < h->tabs.dx.size(); ++j)
        row_slip = std::max(row_slip, std::fabs(h->tabs.dx[j] - h->tabs.dx[j - 1]));
    row_slip *= kDeg2Rad * (1.0 + 1e-9);

    // ---- plan: local geometry (heuristic inputs only) -> tile shape + lag patch
    Geometry geo;
    {
        const CarrCommon c0 = carr_common(*hdr_small, solar_r);
        const int ic = grid->n_lon / 2, jc = grid->n_lat / 2;
        double a0, a1, b0, b1, c0x, c0y;
        carr_term_host(h->tabs, c0, ic, jc, &a0, &a1);
        carr_term_host(h->tabs, c0, std::min(ic + 1, grid->n_lon - 1), jc, &b0, &b1);
        carr_term_host(h->tabs, c0, ic, std::min(jc + 1, grid->n_lat - 1), &c0x, &c0y);
        geo.dx_di = b0 - a0;
        geo.dy_di = b1 - a1;
        geo.dx_dj = c0x - a0;
        geo.dy_dj = c0y - a1;
        // utils/rectify.py:399-404: X0 = -(c d1 + s d2)/cdelt1, Y0 = -(-s d1 + c d2)/cdelt2
        const double s1 = lag_step(lags->crval1, d.n1), s2 = lag_step(lags->crval2, d.n2);
        geo.ax = c0.cr * s1 / hdr_small->cdelt1;
        geo.ay = c0.sr * s1 / hdr_small->cdelt2;
        geo.bx = c0.sr * s2 / hdr_small->cdelt1;
        geo.by = c0.cr * s2 / hdr_small->cdelt2;
    }
    const Plan plan = plan_sweep(h, geo, call);
    PrecomputeArgs pa;
    int n_tiles;
    RETCHK(setup_precompute(h, plan, method, &pa, &n_tiles));

    // ---- every (cdelt1, cdelt2, crota) combination = one precompute + one sweep launch; all lag parameters of all
    //      launches are staged together and uploaded once
    struct Launch {
        size_t slot_off;
        int n_batches;
        CarrCommon cc;
        double f0lo, f0hi, f1lo, f1hi;
    };
    std::vector<Launch> launches;
    std::vector<double> params;  // per launch: [X0 x ns][Y0 x ns]
    std::vector<long long> outidx;
    SlotList slots;
    for (long long c = 0; c < d.nc; ++c) {
        coreg_wcs2d hc;
        if (!combo_slots(call, *hdr_small, plan, c, &hc, &slots)) continue;
        const size_t ns = slots.i1.size();
        Launch L;
        L.slot_off = outidx.size();
        L.n_batches = slots.n_batches;
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
            const double v1 = hdr_small->crval1 + lags->crval1[slots.i1[s]];  // alignment.py:404
            const double v2 = hdr_small->crval2 + lags->crval2[slots.i2[s]];  // alignment.py:412
            const double dx = rc * v1 + rs * v2;
            const double dy = -rs * v1 + rc * v2;
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
        L.f0hi = (double)(h->sW - 1) - x0min;
        L.f1lo = -y0max;
        L.f1hi = (double)(h->sH - 1) - y0min;
        launches.push_back(L);
    }
    if (launches.empty()) return close_empty_sweep(h, call);
    RETCHK(upload_plan(h, params, outidx, call.out_dev, call.n_out));
    RETCHK(prepare_sharded(h, outidx.size(), call.n_out, lag_begin));
    for (const Launch& L : launches) {
        set_carr_common(&cd, L.cc);
        pa.carr = cd;
        pa.f0lo = L.f0lo;
        pa.f0hi = L.f0hi;
        pa.f1lo = L.f1lo;
        pa.f1hi = L.f1hi;
        {
            // whole-tile skip bound (k_precompute): pixels per radian of grid-point motion, grid steps in radians
            const double dm1 = L.cc.dist - 1.0;
            pa.tile_skip = (h->opt_tile_skip && dm1 > 0.0) ? 1 : 0;
            const double per_rad = pa.tile_skip ? (1.0 / dm1 + 1.0 / (dm1 * dm1)) * kRad2Deg * 3600.0 : 0.0;
            pa.lip_x = per_rad / std::fabs(L.cc.cdelt1) * (1.0 + 1e-9);
            pa.lip_y = per_rad / std::fabs(L.cc.cdelt2) * (1.0 + 1e-9);
            // float32 linspace grid: the spacing is uniform to ~1e-7 relative of the coordinate
            pa.dlon = grid->n_lon > 1 ? (std::fabs(grid->lon1 - grid->lon0) / (grid->n_lon - 1) * 1.001 + 1e-4) * kDeg2Rad : 0.0;
            pa.dlat = grid->n_lat > 1 ? (std::fabs(grid->lat1 - grid->lat0) / (grid->n_lat - 1) * 1.001 + 1e-4) * kDeg2Rad : 0.0;
            pa.dlat += row_slip;
        }
        RETCHK(precompute<MODE_TRANSLATE>(h, pa, n_tiles, pick_groups(h, L.n_batches, n_tiles), L.n_batches));
        SweepLaunchSpec sl = sweep_launch(call, MODE_TRANSLATE, L.slot_off, L.n_batches, n_tiles);
        sl.pitch_sel = pick_pitch(h, plan, h->opt_use_lds ? lds_window_elems(h) : 0, order);
        RETCHK(launch_sweep(h, sl));
    }
    return close_sweep(h, call);
}

// Plate-carree maps on both sides (Alignment.align_using_initial_carrington, alignment.py:344-399 ->
// _interpolate_on_large_data_grid :1018-1029 with WCS(CRLN-CAR)): the per-lag map is a rotation of the sphere between
// the native frames of the two maps (a CRVAL2 lag makes the shifted map oblique).  One precompute (native angles of
// the target pixels), one sweep launch per (cdelt1, cdelt2, crota) combination (its native -> pixel affine map is a
// launch constant).  Lags whose header has no valid native pole get NaN (astropy raises for them).
static int sweep_car(coreg_handle* h, const SweepCall& call, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr_small) {
    const coreg_lags* lags = call.lags;
    const LagDims& d = call.d;
    const int order = call.order;
    Mat3 r_target;
    if (car_native_to_celestial(*hdr_target, &r_target))
        return fail(h, COREG_EINVAL, "hdr_target: no valid native pole for this CRVAL2 / LONPOLE (CAR)");
    auto shifted_by = [&](const coreg_wcs2d& base, double v1, double v2) {
        coreg_wcs2d hl = base;
        hl.crval1 = hdr_small->crval1 + v1;  // alignment.py:404
        hl.crval2 = hdr_small->crval2 + v2;  // alignment.py:412
        return hl;
    };
    auto shifted = [&](const coreg_wcs2d& base, int i1, int i2) {
        return shifted_by(base, lags->crval1[i1], lags->crval2[i2]);
    };
    const Plan plan = plan_sweep(h, local_geometry(*hdr_target, call, [&](double v1, double v2, double u, double v,
                                                                        double* x, double* y) {
        CarMapHost m;
        if (m.init(*hdr_target, shifted_by(*hdr_small, v1, v2))) return false;
        m.apply(u, v, x, y);
        return true;
    }), call);

    // rotation of every (CRVAL1, CRVAL2) lag: R = R_small(lag)^T * R_target  (PC / CDELT do not enter it)
    const int i1_lo = call.i1_lo(), i1_hi = call.i1_hi();
    std::vector<double> rot((size_t)(i1_hi - i1_lo + 1) * d.n2 * 9);
    const double nanv = std::numeric_limits<double>::quiet_NaN();
    for (int i1 = i1_lo; i1 <= i1_hi; ++i1)
        for (int i2 = 0; i2 < d.n2; ++i2) {
            double* r = &rot[((size_t)(i1 - i1_lo) * d.n2 + i2) * 9];
            Mat3 rs;
            if (car_native_to_celestial(shifted(*hdr_small, i1, i2), &rs)) {
                for (int k = 0; k < 9; ++k) r[k] = nanv;
                continue;
            }
            const Mat3 m = mat_mul(mat_T(rs), r_target);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) r[3 * a + b] = (double)m.m[a][b];
        }

    struct Launch {
        size_t slot_off;
        int n_batches;
        LaunchU inv;
        bool identity;  // the one-slot launch of the identity lag-point (below)
        // the single-sample pass of this launch: the combination's header, the CRVAL lag indices of its
        // slots, and the slots the scan skips -- all but the lags that leave CRVAL1 or CRVAL2 of the target header alone:
        // only those bring whole rows or columns of coordinates (or, with a CROTA / CDELT lag on top, the reference pixel)
        // back within wcslib's noise of integers
        coreg_wcs2d hc;
        std::vector<int> i1, i2;
        std::vector<unsigned char> tap_skip;
        bool tap_any = false;
    };
    std::vector<Launch> launches;
    std::vector<double> params;  // per launch: SoA [9][slots of the launch]
    std::vector<long long> outidx;
    SlotList slots;
    // The identity lag-point (shifted header == target header: the zero lag of the sub-map semantics, where the target IS
    // the header of the map to align).  The reference's pixel -> world -> pixel round trip (alignment.py:1038-1069) returns
    // i + eps there and the sign of wcslib's rounding noise decides the bounds rule on every border pixel (and, for odd
    // spline orders, the tap set of every pixel).  The sphere rotation of this path cannot even return exact integers, so
    // that lag-point is taken out of the CAR launch and swept on its own with the EXACT identity map by the
    // helioprojective kernels, whose zero-lag machinery (k_border_fix / k_parity_fix) then applies what wcslib's chain
    // (geometry.hpp WcslibCar, bit-exact) decides.  "border_fix" 0: rotation path for that lag-point too.
    long long identity_out = -1;
    BorderFix id_fix;
    std::vector<std::vector<unsigned char>> id_flags;
    auto same_header = [](const coreg_wcs2d& a, const coreg_wcs2d& b) {
        auto eq = [](double x, double y) { return x == y || (x != x && y != y); };
        return a.proj == b.proj && a.crpix1 == b.crpix1 && a.crpix2 == b.crpix2 && a.crval1 == b.crval1 &&
               a.crval2 == b.crval2 && a.cdelt1 == b.cdelt1 && a.cdelt2 == b.cdelt2 && a.pc1_1 == b.pc1_1 &&
               a.pc1_2 == b.pc1_2 && a.pc2_1 == b.pc2_1 && a.pc2_2 == b.pc2_2 && a.unit_to_deg == b.unit_to_deg &&
               eq(a.lonpole, b.lonpole) && eq(a.latpole, b.latpole) && a.naxis1 == b.naxis1 && a.naxis2 == b.naxis2;
    };
    for (long long c = 0; c < d.nc; ++c) {
        coreg_wcs2d hc;
        if (!combo_slots(call, *hdr_small, plan, c, &hc, &slots)) continue;
        const size_t ns = slots.i1.size();
        Launch L;
        L.slot_off = outidx.size();
        L.n_batches = slots.n_batches;
        std::memset(&L.inv, 0, sizeof(L.inv));
        set_affine(&L.inv, car_native_to_pix(hc));
        L.inv.box_c = car_box_c(*hdr_target, hc, plan.tile_w);
        L.inv.pole_sep = 0.0;  // largest over the lags of this launch (below)
        L.identity = false;
        const size_t pbase = params.size();
        params.resize(pbase + 9 * ns);
        for (size_t s = 0; s < ns; ++s) {
            bool pad = slots.outidx[s] < 0;
            if (!pad && h->opt_border_fix && identity_out < 0 && h->gW == h->sW && h->gH == h->sH) {
                const coreg_wcs2d hl = shifted(hc, slots.i1[s], slots.i2[s]);
                if (same_header(hl, *hdr_target)) {
                    identity_out = slots.outidx[s];
                    slots.outidx[s] = -1;  // not this launch's: padding lane (NaN map, nothing written)
                    pad = true;
                }
            }
            const double* r = &rot[((size_t)(slots.i1[s] - i1_lo) * d.n2 + slots.i2[s]) * 9];
            for (int k = 0; k < 9; ++k) params[pbase + (size_t)k * ns + s] = pad ? nanv : r[k];
            if (!pad && r[8] == r[8]) L.inv.pole_sep = std::max(L.inv.pole_sep, car_pole_sep(r));
            unsigned char skip = 1;
            if (!pad && h->opt_tap_fix && r[8] == r[8] && h->gW == h->sW && h->gH == h->sH) {
                // (a CROTA / CDELT lag on top of it included: with both CRVAL equal the map is affine about CRPIX and
                // returns the reference pixel itself to within the noise)
                const coreg_wcs2d hl = shifted(hc, slots.i1[s], slots.i2[s]);
                if (hl.crval1 == hdr_target->crval1 || hl.crval2 == hdr_target->crval2) skip = 0;
            }
            L.tap_skip.push_back(skip);
            L.tap_any = L.tap_any || !skip;
        }
        L.hc = hc;
        L.i1 = slots.i1;
        L.i2 = slots.i2;
        outidx.insert(outidx.end(), slots.outidx.begin(), slots.outidx.end());
        launches.push_back(L);
    }
    if (identity_out >= 0) {
        // one batch, one live slot: the identity homography (every sample ON its pixel); the others are padding
        Launch L;
        std::memset(&L.inv, 0, sizeof(L.inv));
        L.slot_off = outidx.size();
        L.n_batches = 1;
        L.identity = true;
        const size_t ns = kBlock, pbase = params.size();
        params.resize(pbase + 9 * ns, nanv);
        const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int k = 0; k < 9; ++k) params[pbase + (size_t)k * ns] = ident[k];
        outidx.push_back(identity_out);
        outidx.insert(outidx.end(), ns - 1, -1);
        launches.push_back(L);
        {   // (on every rank of a grid-sharded sweep: launch_sweep applies it on rank 0 only, but all must agree that this
            // launch carries a correction)
            AxisInvariance inv;
            inv.rows = inv.cols = true;
            BorderFix::Item it;
            it.slot = 0;
            it.first = 0;
            wcslib_dropped_border_pixels(h, *hdr_target, *hdr_target, inv, &id_fix.pixels);
            it.n = (int)id_fix.pixels.size();
            it.flags_off = -1;
            if (order & 1) {
                it.flags_off = 0;
                id_flags.push_back(wcslib_tap_shift_flags(h, *hdr_target, *hdr_target, inv));
            }
            if (it.n > 0 || it.flags_off >= 0) id_fix.items.push_back(it);
        }
    }
    if (launches.empty()) return close_empty_sweep(h, call);
    trace("sweep_helioprojective: lane parameters laid out");
    RETCHK(upload_plan(h, params, outidx, call.out_dev, call.n_out));
    RETCHK(prepare_sharded(h, outidx.size(), call.n_out, call.lag_begin));
    trace("sweep_helioprojective: plan in page-locked memory");

    PrecomputeArgs pa;
    int n_tiles;
    RETCHK(setup_precompute(h, plan, call.method, &pa, &n_tiles));
    set_affine(&pa.car_fwd, car_pix_to_native(*hdr_target));
    const double inf = std::numeric_limits<double>::infinity();
    pa.f0lo = pa.f1lo = -inf;  // no culling by position: only non-finite reference values drop out
    pa.f0hi = pa.f1hi = inf;
    if (!id_fix.items.empty()) RETCHK(upload_border_pixels(h, id_fix.pixels));
    RETCHK(upload_border_flags(h, id_flags));
    int last_groups = -1, last_batches = -1;
    for (const Launch& L : launches) {
        if (L.identity) {
            // target pixel -> the same pixel of the map to align: base coordinates = pixel indices, no culling by position
            PrecomputeArgs pi = pa;
            std::memset(&pi.car_fwd, 0, sizeof(pi.car_fwd));
            RETCHK(precompute<MODE_HOMOGRAPHY>(h, pi, n_tiles, pick_groups(h, 1, n_tiles), 1));
            last_groups = last_batches = -1;  // (the compacted points now hold pixel indices, not unit vectors)
            SweepLaunchSpec sl = sweep_launch(call, MODE_HOMOGRAPHY, L.slot_off, 1, n_tiles);
            sl.fix = &id_fix;
            RETCHK(launch_sweep(h, sl));
            continue;
        }
        // the work partition (k_tile_list) depends on the group count of the launch: redo it only when that changes
        const int ng = pick_groups(h, L.n_batches, n_tiles);
        RETCHK(precompute<MODE_CAR>(h, pa, n_tiles, ng, L.n_batches, ng != last_groups || L.n_batches != last_batches));
        last_groups = ng;
        last_batches = L.n_batches;
        BorderFix tap;  // (no whole-grid items here: the identity lag has its own launch)
        if (L.tap_any) {
            const double box[4] = {0.0, (double)(h->gW - 1), 0.0, (double)(h->gH - 1)};
            h->tap_last[0] = h->tap_last[1] = h->tap_last[2] = 0;
            RETCHK(prepare_tap_fix(
                h, MODE_CAR, order, *hdr_target, (long long)L.tap_skip.size(), L.tap_skip, box,
                [&](int slot) { return shifted(L.hc, L.i1[(size_t)slot], L.i2[(size_t)slot]); }, &tap,
                h->lane_params.as<double>() + 9 * L.slot_off, &L.inv, &pa.car_fwd));
        }
        SweepLaunchSpec sl = sweep_launch(call, MODE_CAR, L.slot_off, L.n_batches, n_tiles);
        sl.car_inv = &L.inv;
        sl.fix = L.tap_any ? &tap : nullptr;
        RETCHK(launch_sweep(h, sl));
    }
    return close_sweep(h, call);
}

int coreg_sweep_helioprojective(coreg_handle* h, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr_small,
                                const coreg_lags* lags, int order, int method, int cdelt_semantics, int64_t lag_begin,
                                int64_t lag_end, double* corr_out, int out_on_device) {
    if (!h) return COREG_EINVAL;
    const ComboRange combo = take_combo_range(h);
    if (!hdr_target || !hdr_small) return fail(h, COREG_EINVAL, "sweep_helioprojective: null header");
    if (hdr_target->proj != hdr_small->proj || (hdr_small->proj != COREG_PROJ_TAN && hdr_small->proj != COREG_PROJ_CAR))
        return fail(h, COREG_ENOTIMPL, "both headers must be TAN (helioprojective) or both CAR (Carrington maps)");
    auto own_checks = [&] {
        RETCHK(check_wcs(h, hdr_target, false));
        return check_wcs(h, hdr_small, false);
    };
    SweepCall call;
    RETCHK(open_sweep(h, combo, own_checks, lags, order, method, cdelt_semantics, lag_begin, lag_end,
                      hdr_target->naxis1, hdr_target->naxis2, "hdr_target NAXIS1/NAXIS2", corr_out, out_on_device, &call));
    if (call.n_out == 0) return close_sweep(h, call);  // (nothing to fill)
    if (hdr_small->proj == COREG_PROJ_CAR) return sweep_car(h, call, hdr_target, hdr_small);
    const LagDims& d = call.d;

    trace("sweep_helioprojective: enter (checks done)");
    const Plan plan = plan_sweep(h, local_geometry(*hdr_target, call, [&](double v1, double v2, double u, double v,
                                                                        double* x, double* y) {
        coreg_wcs2d hl = *hdr_small;
        hl.crval1 = hdr_small->crval1 + v1;
        hl.crval2 = hdr_small->crval2 + v2;
        double hm[9];
        homography(*hdr_target, hl, hm);
        apply_h(hm, u, v, x, y);
        return true;
    }), call);

    // ---- all slots of all (cdelt1, cdelt2, crota) combinations -> ONE launch
    // Two passes.  (1) per combination, independent of every other and of the handle -- a few host threads share them
    // when the lag set is large (cfg4: 21 combinations x 3 721 lag-points, 1.4 ms of 3 x 3 products on one core):
    // shifted header, slots, one homography per slot, the combination's corner of the cull box.  (2) in combination
    // order, on this thread: the lag-points decided by wcslib's rounding noise (handle caches), the bookkeeping of the
    // odd-order pass, the concatenation.
    std::vector<long long> outidx;
    int n_batches = 0;
    double fx0 = 1e300, fx1 = -1e300, fy0 = 1e300, fy1 = -1e300;  // cull box in target pixels
    HomographyFamily fam;
    fam.init(*hdr_target, *hdr_small, lags->crval1, d.n1, lags->crval2, d.n2, d.nc > 1);
    BorderFix fix;
    std::vector<std::vector<unsigned char>> flags_host;  // per noise-decided lag-point (odd spline orders only)
    // odd spline orders: what prepare_tap_fix needs to rebuild a slot's shifted header
    // (grid shares across GPUs: every rank lists the samples -- the re-evaluation of a flagged lag-point needs them on
    // every rank; the correction itself is launched on rank 0 only, launch_sweep)
    // Odd orders: every sample within 1e-8 px of an integer coordinate (the sign of wcslib's noise picks the taps); even
    // orders: only those within 1e-8 px of a BOUND of the image (the sign decides the bounds rule) -- a pure CRVAL1 or
    // CRVAL2 lag under an unrotated header keeps whole border rows / columns of the grid there.
    const bool tap_fixing = h->opt_tap_fix != 0;
    std::vector<coreg_wcs2d> tap_combo;      // the (cdelt, crota)-shifted header of each combination
    std::vector<int> tap_slot_combo, tap_slot_i1, tap_slot_i2;
    std::vector<unsigned char> tap_skip;     // padding lanes and lag-points the structured fix handles
    const int i1_lo = call.i1_lo(), i1_hi = call.i1_hi();
    fam.fill_products(i1_lo, i1_hi);  // (read-only from here on: `get` is safe to call from several threads)
    const double nanv = std::numeric_limits<double>::quiet_NaN();
    struct ComboPlan {
        bool used = false;
        coreg_wcs2d hc;
        SlotList slots;
        std::vector<double> hs;  // AoS [slot][9]
        double box[4] = {1e300, -1e300, 1e300, -1e300};
    };
    std::vector<ComboPlan> cps((size_t)d.nc);
    // which target pixels can ever be in bounds: inverse maps of the small image's corners for the lags on the
    // boundary of the (CRVAL1, CRVAL2) rectangle, chosen BY VALUE (the reference accepts lag lists in any order):
    // smallest, largest and the value nearest the middle of each axis (the maps vary smoothly and monotonically
    // with the lag value, the +-3 px margin below covers the curvature in between)
    int e1[3], e2[3];
    extreme_lags(lags->crval1 + i1_lo, i1_hi - i1_lo + 1, e1);
    extreme_lags(lags->crval2, d.n2, e2);
    auto plan_combo = [&](long long c) {
        ComboPlan& cp = cps[(size_t)c];
        cp.used = combo_slots(call, *hdr_small, plan, c, &cp.hc, &cp.slots);
        if (!cp.used) return;
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
                hl.crval1 = hdr_small->crval1 + lags->crval1[i1_lo + e1[a1]];
                hl.crval2 = hdr_small->crval2 + lags->crval2[e2[a2]];
                double hi[9];
                homography(hl, *hdr_target, hi);
                for (int k = 0; k < 4; ++k) {
                    double px, py;
                    apply_h(hi, (k & 1) ? (double)(h->sW - 1) : 0.0, (k & 2) ? (double)(h->sH - 1) : 0.0, &px, &py);
                    cp.box[0] = std::min(cp.box[0], px);
                    cp.box[1] = std::max(cp.box[1], px);
                    cp.box[2] = std::min(cp.box[2], py);
                    cp.box[3] = std::max(cp.box[3], py);
                }
            }
    };
    trace("sweep_helioprojective: geometry + lag family ready");
    const unsigned plan_threads = (d.nc >= 2 && (long long)d.nc * d.n1 * d.n2 >= 16384) ? 8u : 1u;
    parallel_for(d.nc, plan_threads, 1, [&](long long lo, long long hi) {
        for (long long c = lo; c < hi; ++c) plan_combo(c);
    });
    for (long long c = 0; c < d.nc; ++c) {
        ComboPlan& cp = cps[(size_t)c];
        if (!cp.used) continue;
        const SlotList& slots = cp.slots;
        const coreg_wcs2d& hc = cp.hc;
        if (tap_fixing) {
            tap_combo.push_back(hc);
            for (size_t s = 0; s < slots.i1.size(); ++s) {
                tap_slot_combo.push_back((int)tap_combo.size() - 1);
                tap_slot_i1.push_back(slots.outidx[s] < 0 ? 0 : slots.i1[s]);
                tap_slot_i2.push_back(slots.outidx[s] < 0 ? 0 : slots.i2[s]);
                tap_skip.push_back(slots.outidx[s] < 0 ? 1 : 0);
            }
        }
        if (h->opt_border_fix) {
            for (size_t s = 0; s < slots.i1.size(); ++s) {
                if (slots.outidx[s] < 0) continue;
                // same tangent point as the target (sub-map path, zero CRVAL lag) and an invariant image axis: exact
                // invariant map on the device, border pixels decided as the reference's wcslib round trip decides them
                // (geometry.hpp WcslibTan, k_border_fix).  (The tangent points are compared first: every other
                // lag-point is dismissed without building its header.)
                const double v1 = hdr_small->crval1 + lags->crval1[slots.i1[s]];
                const double v2 = hdr_small->crval2 + lags->crval2[slots.i2[s]];
                if (v1 != hdr_target->crval1 || v2 != hdr_target->crval2) continue;
                coreg_wcs2d hl = hc;
                hl.crval1 = v1;
                hl.crval2 = v2;
                double* hm = &cp.hs[9 * s];
                const AxisInvariance inv = snap_invariant_axes(*hdr_target, hl, h->gW, h->gH, hm);
                if (inv.rows || inv.cols) {
                    BorderFix::Item it;
                    it.slot = (long long)(outidx.size() + s);
                    it.first = (int)fix.pixels.size();
                    wcslib_dropped_border_pixels(h, *hdr_target, hl, inv, &fix.pixels);
                    it.n = (int)fix.pixels.size() - it.first;
                    it.flags_off = -1;
                    if (order & 1) {
                        it.flags_off = (long long)flags_host.size() * h->gW * h->gH;
                        flags_host.push_back(wcslib_tap_shift_flags(h, *hdr_target, hl, inv));  // (copy: the cache may evict)
                    }
                    if (it.n > 0 || it.flags_off >= 0) fix.items.push_back(it);
                    if (tap_fixing) tap_skip[(size_t)it.slot] = 1;  // (its whole grid sits on integers: k_parity_fix)
                }
            }
        }
        fx0 = std::min(fx0, cp.box[0]);
        fx1 = std::max(fx1, cp.box[1]);
        fy0 = std::min(fy0, cp.box[2]);
        fy1 = std::max(fy1, cp.box[3]);
        outidx.insert(outidx.end(), slots.outidx.begin(), slots.outidx.end());
        n_batches += slots.n_batches;
    }
    if (n_batches == 0) return close_empty_sweep(h, call);
    trace("sweep_helioprojective: combinations planned");
    const size_t ns = outidx.size();
    std::vector<double> params(9 * ns);
    double eps_max = 0.0;  // largest |h6 x + h7 y| over the target grid and all lags
    {
        // AoS per combination -> SoA [9][ns] of the launch, the same threads over the combinations
        std::vector<size_t> off((size_t)d.nc + 1, 0);
        for (long long c = 0; c < d.nc; ++c) off[(size_t)c + 1] = off[(size_t)c] + (cps[(size_t)c].used ? cps[(size_t)c].slots.i1.size() : 0);
        std::vector<double> eps_of((size_t)d.nc, 0.0);
        auto transpose = [&](long long c) {
            const ComboPlan& cp = cps[(size_t)c];
            if (!cp.used) return;
            const size_t n = cp.slots.i1.size(), at = off[(size_t)c];
            double em = 0.0;
            for (size_t s = 0; s < n; ++s) {
                const double* hm = &cp.hs[9 * s];
                for (int k = 0; k < 9; ++k) params[(size_t)k * ns + at + s] = hm[k];
                const double e = std::fabs(hm[6]) * (double)h->gW + std::fabs(hm[7]) * (double)h->gH;
                if (e == e) em = std::max(em, e);
            }
            eps_of[(size_t)c] = em;
        };
        parallel_for(d.nc, plan_threads, 1, [&](long long lo, long long hi) {
            for (long long c = lo; c < hi; ++c) transpose(c);
        });
        for (double e : eps_of) eps_max = std::max(eps_max, e);
    }
    // 1/(1 + eps) = 1 - eps + eps^2 is exact to float64 below ~4e-6 (eps^3 < 1e-16); wider fields divide exactly
    const int sweep_mode = (h->opt_h_series && eps_max < 4.0e-6) ? MODE_HOMOGRAPHY_SERIES : MODE_HOMOGRAPHY;
    RETCHK(upload_plan(h, params, outidx, call.out_dev, call.n_out));
    RETCHK(prepare_sharded(h, outidx.size(), call.n_out, lag_begin));

    PrecomputeArgs pa;
    int n_tiles;
    RETCHK(setup_precompute(h, plan, method, &pa, &n_tiles));
    // the maps are projective and the image corners bound its interior
    pa.f0lo = std::floor(fx0) - 3.0;
    pa.f0hi = std::ceil(fx1) + 3.0;
    pa.f1lo = std::floor(fy0) - 3.0;
    pa.f1hi = std::ceil(fy1) + 3.0;
    if (!fix.items.empty()) RETCHK(upload_border_pixels(h, fix.pixels));
    RETCHK(upload_border_flags(h, flags_host));
    RETCHK(precompute<MODE_HOMOGRAPHY>(h, pa, n_tiles, pick_groups(h, n_batches, n_tiles), n_batches));
    h->tap_last[0] = h->tap_last[1] = h->tap_last[2] = 0;
    const double tap_box[4] = {pa.f0lo, pa.f0hi, pa.f1lo, pa.f1hi};
    trace("sweep_helioprojective: precompute launched");
    if (tap_fixing)
        RETCHK(prepare_tap_fix(
            h, sweep_mode, order, *hdr_target, (long long)ns, tap_skip, tap_box,
            [&](int slot) {
                coreg_wcs2d hl = tap_combo[(size_t)tap_slot_combo[(size_t)slot]];
                hl.crval1 = hdr_small->crval1 + lags->crval1[tap_slot_i1[(size_t)slot]];
                hl.crval2 = hdr_small->crval2 + lags->crval2[tap_slot_i2[(size_t)slot]];
                return hl;
            },
            &fix));
    trace("sweep_helioprojective: single-sample scan done");
    SweepLaunchSpec sl = sweep_launch(call, sweep_mode, 0, n_batches, n_tiles);
    sl.fix = &fix;
    sl.pitch_sel = pick_pitch(h, plan, h->opt_use_lds ? lds_window_elems(h) : 0, order);
    RETCHK(launch_sweep(h, sl));
    return close_sweep(h, call);
}


int coreg_sums_size(coreg_handle* h, int64_t* n_doubles) {
    if (!h || !n_doubles) return COREG_EINVAL;
    *n_doubles = (int64_t)h->sums_slots * kNumSums;
    return COREG_OK;
}

int coreg_copy_sums(coreg_handle* h, double* dst, int dst_on_device) {
    if (!h || !dst) return COREG_EINVAL;
    if (h->sums_slots <= 0 || h->pending_fin.empty()) return fail(h, COREG_ESTATE, "no point-sharded sweep is pending");
    RETCHK(bind_device(h));
    const size_t bytes = (size_t)h->sums_slots * kNumSums * sizeof(double);
    HIPCHK(hipMemcpyAsync(dst, h->sums.p, bytes, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          h->stream));
    if (!dst_on_device) HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_finalize_sums(coreg_handle* h, const double* sums, int sums_on_device, double* corr_out, int out_on_device) {
    if (!h || !sums) return COREG_EINVAL;
    if (h->sums_slots <= 0 || h->pending_fin.empty()) return fail(h, COREG_ESTATE, "no point-sharded sweep is pending");
    if (!corr_out && h->pending_n_out > 0) return fail(h, COREG_EINVAL, "corr_out is null");
    RETCHK(bind_device(h));
    const long long n_out = h->pending_n_out;
    const size_t bytes = (size_t)h->sums_slots * kNumSums * sizeof(double);
    if ((const void*)sums != h->sums.p) {
        HIPCHK(hipMemcpyAsync(h->sums.p, sums, bytes, sums_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              h->stream));
        // a host buffer belongs to the caller again on return (with a device destination nothing below waits)
        if (!sums_on_device) HIPCHK(hipStreamSynchronize(h->stream));
    }
    double* out_dev = corr_out;
    if (!out_on_device) {
        HIPCHK(h->out_dev.reserve((size_t)std::max<long long>(n_out, 1) * sizeof(double)));
        out_dev = h->out_dev.as<double>();
    }
    if (n_out > 0) {
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, h->stream, out_dev,
                           (long long)n_out, std::numeric_limits<double>::quiet_NaN());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(h->counts.reserve((size_t)std::max<long long>(n_out, 1) * sizeof(double)));
    h->counts_n = n_out;
    RETCHK(fill_nan(h, h->counts.as<double>(), n_out));
    const size_t n_pending = h->pending_fin.size();
    size_t points_of = n_pending - 1;  // the launch whose compacted points the handle holds: the sweep's last one
    // a plate-carree sweep has one pending launch per combination, and asking each one "anything flagged?"
    // used to cost a host round trip apiece.  With several launches pending, all of them are finalized and their flags
    // COUNTED first (k_refine_list adds into a counter of its own, counters[2]): ONE read-back -- and when the total is
    // zero, the normal case, that was all.  Otherwise the per-launch pass below runs as before (k_finalize is idempotent).
    bool probe_says_nothing_flagged = false;
    if (n_pending > 1) {
        long long* probe = h->counters.as<long long>() + 2;
        HIPCHK(hipMemsetAsync(probe, 0, sizeof(long long), h->stream));
        for (size_t ip = 0; ip < n_pending; ++ip) {
            const coreg_handle::PendingFinalize& pf = h->pending_fin[ip];
            // (the counters of the sweep are written by the pass that re-evaluates)
            FinalizeArgs f;
            RETCHK(finalize_pending(h, pf, nullptr, out_dev, &f));
            if (f.refine.enabled)
                hipLaunchKernelGGL(k_refine_list, dim3(1), dim3(kListThreads), 0, h->stream, f.refine, pf.n_slots, probe);
        }
        HIPCHK(hipGetLastError());
        long long flagged = 0;
        HIPCHK(hipMemcpyAsync(&flagged, probe, sizeof(flagged), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        probe_says_nothing_flagged = flagged == 0;
    }
    for (size_t ip = 0; ip < n_pending && !probe_says_nothing_flagged; ++ip) {
        const coreg_handle::PendingFinalize& pf = h->pending_fin[ip];
        // flags from the REDUCED sums: the same on every rank
        FinalizeArgs f;
        RETCHK(finalize_pending(h, pf, h->counters.as<long long>(), out_dev, &f));
        const RefineArgs rf = f.refine;
        if (!rf.enabled) continue;
        // Ill-conditioned lag-points: every rank holds both images and re-evaluates them over the WHOLE grid (not its
        // share) with the same kernels in the same order -- identical coefficients on every rank, and equal to the
        // single-GPU sweep's, without a second collective.  The compacted points of a launch that was not the sweep's
        // last have been overwritten by the later launches: computed again, only when something is flagged.
        hipLaunchKernelGGL(k_refine_list, dim3(1), dim3(kListThreads), 0, h->stream, rf, pf.n_slots, h->counters.as<long long>());
        HIPCHK(hipGetLastError());
        int head[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(head, rf.head, sizeof(head), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (head[0] == 0) continue;
        if (points_of != ip && pf.replay_precompute) {
            RETCHK(pf.replay_precompute(h));
            points_of = ip;
        }
        // (with the launch's noise-decided samples about the flagged slots' own pivots, as launch_sweep does on one GPU)
        RETCHK(refine_with_fixes(h, rf, pf.fixes, pf.n_slots, f.out_index, pf.lag_begin, out_dev));
    }
    HIPCHK(hipGetLastError());
    if (!out_on_device && n_out > 0) {
        HIPCHK(hipMemcpyAsync(corr_out, out_dev, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return COREG_OK;
}

int coreg_get_pivots(coreg_handle* h, double* pivots2) {
    if (!h || !pivots2) return COREG_EINVAL;
    RETCHK(bind_device(h));
    HIPCHK(hipMemcpyAsync(pivots2, h->pivots.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_set_pivots(coreg_handle* h, const double* pivots2) {
    if (!h || !pivots2) return COREG_EINVAL;
    if (!(pivots2[0] == pivots2[0]) || !(pivots2[1] == pivots2[1]) || std::isinf(pivots2[0]) || std::isinf(pivots2[1]))
        return fail(h, COREG_EINVAL, "set_pivots: pivots must be finite");
    RETCHK(bind_device(h));
    HIPCHK(hipMemcpyAsync(h->pivots.p, pivots2, 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // the caller's two doubles are free again on return
    return COREG_OK;
}

int coreg_last_counts(coreg_handle* h, double* dst, int dst_on_device) {
    if (!h) return COREG_EINVAL;
    if (h->counts_n < 0) return fail(h, COREG_ESTATE, "last_counts: no sweep has run on this handle");
    if (!dst && h->counts_n > 0) return fail(h, COREG_EINVAL, "last_counts: dst is null");
    RETCHK(bind_device(h));
    if (h->counts_n > 0)
        HIPCHK(hipMemcpyAsync(dst, h->counts.p, (size_t)h->counts_n * sizeof(double),
                              dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_last_stats(coreg_handle* h, coreg_stats* out) {
    if (!h || !out) return COREG_EINVAL;
    RETCHK(bind_device(h));
    RETCHK(collect_stats(h));  // waits for an in-flight device-output sweep
    *out = h->stats;
    return COREG_OK;
}

}  // extern "C"
