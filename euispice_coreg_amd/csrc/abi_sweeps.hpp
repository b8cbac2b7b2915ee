// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): C ABI: coreg_sweep_carrington / coreg_sweep_helioprojective (each launch described by a SweepLaunchSpec),
// grid-shared sums, pivots, stats.
#pragma once
namespace {
// ---- the steps every sweep shares ---------------------------------------------------------------------------------
// An entry point = its checks (open_sweep), the Carrington table upload where it has one, its planner (sweep_plan.hpp:
// what to launch, decided on the host without the device) and run_sweep_plan (the one launch loop).

// The method of a header-shift sweep.  mi_ok: the entry point has a mutual-information score (the Carrington sweep alone:
// its plans have no noise-decided samples, and the corrections of the others are slabs of Pearson sums, sweep_plan.hpp);
// it is then refused here for what it lacks on this handle -- a grid share, its bins (host_sweep_mi.hpp).
int check_method(coreg_handle* h, int method, bool mi_ok) {
    if (method == COREG_METHOD_MUTUAL_INFORMATION) {
        if (!mi_ok)
            return fail(h, COREG_ENOTIMPL, "method COREG_METHOD_MUTUAL_INFORMATION is a score of coreg_sweep_carrington only: the "
                                           "noise-decided samples of the other header-shift sweeps are corrected as Pearson sums");
        return check_sweep_mi(h);
    }
    if (method != COREG_METHOD_CORRELATION && method != COREG_METHOD_RESIDUS && method != COREG_METHOD_RESIDUS_MASKED)
        return fail(h, COREG_ENOTIMPL,
                    "method must be COREG_METHOD_CORRELATION, COREG_METHOD_RESIDUS or COREG_METHOD_RESIDUS_MASKED");
    return COREG_OK;
}

// The checks and set-up of the public sweeps, in this order: method (check_method), order, the entry point's own checks (`own_checks`),
// the lag set with the combination range the entry point took off the handle, the device, the reference-on-grid shape
// (`grid_w` x `grid_h`, `grid_what` names it), begin_sweep.  With nothing to sweep (call->n_out == 0) the caller returns
// end_sweep at once.
template <typename OwnChecks>
int open_sweep(coreg_handle* h, ComboRange combo, OwnChecks own_checks, const coreg_lags* lags, int order, int method,
               bool mi_ok, int sem, int64_t lag_begin, int64_t lag_end, int grid_w, int grid_h, const char* grid_what,
               double* corr_out, int out_on_device, SweepCall* call) {
    RETCHK(check_method(h, method, mi_ok));
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

// the precompute of a launch of sweep mode `mode` (both homography modes share MODE_HOMOGRAPHY's)
int precompute_for(coreg_handle* h, int mode, const PrecomputeArgs& pa, int n_tiles, const PlannedLaunch& L) {
    if (mode == MODE_TRANSLATE) return precompute<MODE_TRANSLATE>(h, pa, n_tiles, L.n_groups, L.n_batches, L.precompute);
    if (mode != MODE_CAR) return precompute<MODE_HOMOGRAPHY>(h, pa, n_tiles, L.n_groups, L.n_batches, L.precompute);
    return precompute<MODE_CAR>(h, pa, n_tiles, L.n_groups, L.n_batches, L.precompute);
}

// The launch of `call` whose slots start at slot `slot_off` of the uploaded plan; run_sweep_plan adds what the plan says
// of it (car_inv, fix, pitch_sel).
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

// The one launch loop: a plan's parameters, border pixels and flag grids go up once; then every launch is its precompute
// (the plan says whether it must actually run), its single-sample scan where the plan lists samples, and its sweep.
int run_sweep_plan(coreg_handle* h, const SweepCall& call, const SweepPlan& plan) {
    if (plan.error) return fail(h, COREG_EINVAL, plan.error);
    if (plan.empty()) return close_empty_sweep(h, call);
    RETCHK(upload_plan(h, plan.params, plan.outidx, call.out_dev, call.n_out));
    RETCHK(prepare_sharded(h, plan.outidx.size(), call.n_out, call.lag_begin));
    trace("run_sweep_plan: plan in page-locked memory");
    PrecomputeArgs pa0;
    int n_tiles;
    RETCHK(setup_precompute(h, plan.lags, call.method, &pa0, &n_tiles));
    if (!plan.fix.items.empty()) RETCHK(upload_border_pixels(h, plan.fix.pixels));
    RETCHK(upload_border_flags(h, plan.flags));
    for (const PlannedLaunch& L : plan.launches) {
        const bool car = L.mode == MODE_CAR;
        PrecomputeArgs pa = pa0;
        if (L.mode == MODE_TRANSLATE) {
            pa.carr = carr_dev(h);
            set_carr_common(&pa.carr, L.cc);
        }
        pa.car_fwd = L.car_fwd;
        pa.f0lo = L.f0lo;
        pa.f0hi = L.f0hi;
        pa.f1lo = L.f1lo;
        pa.f1hi = L.f1hi;
        pa.tile_skip = L.tile_skip;
        pa.lip_x = L.lip_x;
        pa.lip_y = L.lip_y;
        pa.dlon = L.dlon;
        pa.dlat = L.dlat;
        RETCHK(precompute_for(h, L.mode, pa, n_tiles, L));
        trace("run_sweep_plan: precompute launched");
        BorderFix fix;
        if (L.border_items) fix.border = &plan.fix;
        if (L.scan) {
            h->tap_last[0] = h->tap_last[1] = h->tap_last[2] = 0;
            RETCHK(prepare_tap_fix(
                h, L.mode, call.order, plan.target, (long long)L.tap_skip.size(), L.tap_skip, L.scan_box,
                [&](int slot) { return plan.shifted_of(L, *call.lags, slot); }, &fix,
                h->lane_params.as<double>() + 9 * L.slot_off, car ? &L.car_inv : nullptr, car ? &L.car_fwd : nullptr));
            trace("run_sweep_plan: single-sample scan done");
        }
        SweepLaunchSpec sl = sweep_launch(call, L.mode, L.slot_off, L.n_batches, n_tiles);
        if (call.method == COREG_METHOD_MUTUAL_INFORMATION) {
            // (plan_carrington's launches only: MODE_TRANSLATE, nothing noise-decided, no re-evaluation)
            RETCHK(launch_sweep_mi(h, sl, plan.outidx.data() + L.slot_off));
            continue;
        }
        if (car) sl.car_inv = &L.car_inv;
        sl.fix = &fix;
        sl.pitch_sel = plan.pitch;
        RETCHK(launch_sweep(h, sl));
    }
    return close_sweep(h, call);
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
    RETCHK(open_sweep(h, combo, own_checks, lags, order, method, true, cdelt_semantics, lag_begin, lag_end, grid->n_lon,
                      grid->n_lat, "the Carrington grid", corr_out, out_on_device, &call));
    if (call.n_out == 0) return close_sweep(h, call);  // (nothing to fill)
    RETCHK(upload_carr_tables(h, *grid, *hdr_small, h->has_rot_small ? &h->rot_small : nullptr));
    return run_sweep_plan(h, call, plan_carrington(call, *hdr_small, *grid, solar_r, sweep_env(h)));
}

// Helioprojective (TAN) headers on both sides, or plate-carree (CAR) maps on both sides (sweep_plan.hpp: plan_tan, plan_car)
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
    RETCHK(open_sweep(h, combo, own_checks, lags, order, method, false, cdelt_semantics, lag_begin, lag_end,
                      hdr_target->naxis1, hdr_target->naxis2, "hdr_target NAXIS1/NAXIS2", corr_out, out_on_device, &call));
    if (call.n_out == 0) return close_sweep(h, call);  // (nothing to fill)
    if (hdr_small->proj == COREG_PROJ_CAR) return run_sweep_plan(h, call, plan_car(call, *hdr_target, *hdr_small, sweep_env(h)));
    trace("sweep_helioprojective: enter (checks done)");
    return run_sweep_plan(h, call, plan_tan(call, *hdr_target, *hdr_small, sweep_env(h)));
}

int coreg_sweep_set_bins(coreg_handle* h, const double* edges_small, int32_t n_small, const double* edges_large,
                         int32_t n_large) {
    if (!h) return COREG_EINVAL;
    return sweep_mi_set_bins(h, edges_small, n_small, edges_large, n_large);
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
