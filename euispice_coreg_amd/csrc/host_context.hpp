// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the iterative-context
// sweep (AlignementSpiceIterativeContextRaster): the resident imager frames (ContextState, freed with the handle that owns
// it), the per-lag plan (homographies of every
// (frame, lag) and of the SPICE resample, wcslib's bounds decisions on the grid's border), the launches.
#pragma once

struct ContextState {
    DevBuf frames;  // [n][H][W], float or double as the files store them
    int n = 0, W = 0, H = 0;
    bool f32 = true;
    std::vector<coreg_wcs2d> hdrs;
    bool have_pivot = false;
    double pivot = 0.0;  // mean of the finite frame pixels (pivot of the context sums)
    DevBuf mean, col_frame, h_ctx, h_sp, edge, partials, out_index, flags, slot_pivots, list, head, out_tmp;
    Event ev_a, ev_b;
};

namespace {

constexpr long long kCtxBatch = 8192;  // lag slots per launch (bounds the plan and the partial slabs)
constexpr double kCtxEdgeTol = 1e-6;   // px: a border sample this close to a bound is decided by wcslib's arithmetic

int context_set_frames(coreg_handle* h, int n, int ny, int nx, int dtype, const coreg_wcs2d* hdrs,
                       const void* const* pixels) {
    if (n < 1 || ny < 1 || nx < 1 || !hdrs || (dtype != COREG_F32 && dtype != COREG_F64) || too_many(ny, nx))
        return fail(h, COREG_EINVAL, "set_context_frames: bad arguments");
    for (int k = 0; k < n; ++k) {
        if (const char* why = wcs_problem(hdrs[k], false))
            return fail(h, COREG_EINVAL, std::string("set_context_frames: frame header: ") + why);
        if (hdrs[k].proj != COREG_PROJ_TAN) return fail(h, COREG_EINVAL, "set_context_frames: frames must be TAN");
    }
    RETCHK(bind_device(h));
    if (!h->ctx) {
        h->ctx.reset(new (std::nothrow) ContextState());
        if (!h->ctx) return fail(h, COREG_ENOMEM, "set_context_frames: out of host memory");
        HIPCHK(hipEventCreate(&h->ctx->ev_a.e));
        HIPCHK(hipEventCreate(&h->ctx->ev_b.e));
    }
    ContextState* c = h->ctx.get();
    const size_t esz = dtype == COREG_F32 ? sizeof(float) : sizeof(double);
    const size_t per = (size_t)ny * nx * esz;
    HIPCHK(hipStreamSynchronize(h->stream));  // (a sweep in flight may still read the old stack)
    HIPCHK(c->frames.reserve(per * n));
    c->n = n;
    c->W = nx;
    c->H = ny;
    c->f32 = dtype == COREG_F32;
    c->hdrs.assign(hdrs, hdrs + n);
    c->have_pivot = false;
    for (int k = 0; k < n; ++k)
        if (pixels && pixels[k]) HIPCHK(hipMemcpy((char*)c->frames.p + per * k, pixels[k], per, hipMemcpyHostToDevice));
    return COREG_OK;
}

int context_frame_from_small(coreg_handle* h, int k) {
    ContextState* c = h->ctx.get();
    if (!c) return fail(h, COREG_ESTATE, "context_frame_from_small: coreg_set_context_frames has not been called");
    if (k < 0 || k >= c->n) return fail(h, COREG_EINVAL, "context_frame_from_small: no such frame");
    if (!h->small.p || h->sW != c->W || h->sH != c->H)
        return fail(h, COREG_EINVAL, "context_frame_from_small: the decoded image does not have the frames' shape");
    if (c->f32 && !h->small_f32)
        return fail(h, COREG_EINVAL, "context_frame_from_small: a float64 image cannot go into a float32 frame stack");
    RETCHK(bind_device(h));
    const long long n = (long long)c->W * c->H;
    const dim3 grid(1024), blk(256);
    if (c->f32)
        hipLaunchKernelGGL((k_ctx_copy_frame<float, float>), grid, blk, 0, h->stream, c->frames.as<float>() + n * k,
                           h->small.as<float>(), n);
    else if (h->small_f32)
        hipLaunchKernelGGL((k_ctx_copy_frame<double, float>), grid, blk, 0, h->stream, c->frames.as<double>() + n * k,
                           h->small.as<float>(), n);
    else
        hipLaunchKernelGGL((k_ctx_copy_frame<double, double>), grid, blk, 0, h->stream, c->frames.as<double>() + n * k,
                           h->small.as<double>(), n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    c->have_pivot = false;
    return COREG_OK;
}

// Plan of slots [s0, s1) of a launch whose first slot is lag index `first`: homographies and border decisions.
void context_plan_range(const ContextState& c, const coreg_wcs2d& target4, const coreg_wcs2d& small,
                        const coreg_lags& lags, const LagDims& d, int sem, long long first, long long s0, long long s1,
                        int sW, int sH, double* h_ctx, double* h_sp, unsigned char* edge) {
    const int gW = small.naxis1, gH = small.naxis2;
    const int ne = 2 * (gW + gH);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (long long s = s0; s < s1; ++s) {
        const long long r = first + s;
        const int i1 = (int)(r / (d.n2 * d.nc)), i2 = (int)(r / d.nc % d.n2);
        int i3, i4, i5;
        d.inner(r % d.nc, &i3, &i4, &i5);
        coreg_wcs2d ctx, grid, shifted;
        const int rc = context_lag_headers(target4, small, lags.crval1[i1], lags.crval2[i2], lags.cdelt1[i3],
                                           lags.cdelt2[i4], lags.crota[i5], sem, &ctx, &grid, &shifted);
        unsigned char* ed = edge + (size_t)s * ne;
        std::memset(ed, 0, ne);
        if (rc) {  // no header to evaluate: every sample NaN, the lag-point NaN
            for (int k = 0; k < 9 * c.n; ++k) h_ctx[(size_t)s * 9 * c.n + k] = nan;
            for (int k = 0; k < 9; ++k) h_sp[(size_t)s * 9 + k] = nan;
            continue;
        }
        for (int f = 0; f < c.n; ++f) homography(ctx, c.hdrs[f], h_ctx + ((size_t)s * c.n + f) * 9);
        double* hs = h_sp + (size_t)s * 9;
        homography(grid, shifted, hs);
        WcslibTan wf, wt;
        bool wcs_ready = false;
        for (int e = 0; e < ne; ++e) {
            int px, py;
            if (e < gH) px = 0, py = e;
            else if (e < 2 * gH) px = gW - 1, py = e - gH;
            else if (e < 2 * gH + gW) px = e - 2 * gH, py = 0;
            else px = e - 2 * gH - gW, py = gH - 1;
            double sx, sy;
            apply_h(hs, (double)px, (double)py, &sx, &sy);
            const bool near = std::fabs(sx) < kCtxEdgeTol || std::fabs(sx - (sW - 1)) < kCtxEdgeTol ||
                              std::fabs(sy) < kCtxEdgeTol || std::fabs(sy - (sH - 1)) < kCtxEdgeTol;
            if (!near) continue;
            if (!wcs_ready) {
                wf.init(grid);
                wt.init(shifted);
                wcs_ready = true;
            }
            double wx, wy;
            wcslib_pixel_to_pixel(wf, wt, (double)px, (double)py, &wx, &wy);
            const bool inside = wx >= 0.0 && wx <= (double)(sW - 1) && wy >= 0.0 && wy <= (double)(sH - 1);
            ed[e] = inside ? 1 : 2;
        }
    }
}

// fn(F(), S()) with F, S the element types of the frame stack and of the SPICE image (float or double)
template <typename Fn>
void context_types(bool frames_f32, bool small_f32, Fn fn) {
    if (frames_f32 && small_f32) fn(float(), float());
    else if (frames_f32) fn(float(), double());
    else if (small_f32) fn(double(), float());
    else fn(double(), double());
}

int context_sweep(coreg_handle* h, const coreg_wcs2d* target4, const coreg_wcs2d* small, const int32_t* col_frame,
                  const coreg_lags* lags, int order, int method, int sem, int has_min, double vmin, int has_max,
                  double vmax, long long lag_begin, long long lag_end, double* corr_out, int out_on_device) {
    // the combination range of a grid-shared sweep does not apply here: refused, and off the handle either way
    const ComboRange combo = take_combo_range(h);
    if (combo.begin != 0 || combo.end != 0)
        return fail(h, COREG_EINVAL, "sweep_context: combo_begin/combo_end do not apply to this sweep");
    if (method == COREG_METHOD_MUTUAL_INFORMATION)
        return fail(h, COREG_ENOTIMPL, "sweep_context: COREG_METHOD_MUTUAL_INFORMATION is a score of coreg_sweep_carrington only");
    ContextState* c = h->ctx.get();
    if (!c) return fail(h, COREG_ESTATE, "sweep_context: coreg_set_context_frames has not been called");
    if (!h->small.p) return fail(h, COREG_ESTATE, "sweep_context: coreg_set_small (the SPICE image) has not been called");
    if (!target4 || !small || !col_frame || !lags) return fail(h, COREG_EINVAL, "sweep_context: null argument");
    for (const coreg_wcs2d* w : {target4, small})
        if (const char* why = wcs_problem(*w, false)) return fail(h, COREG_EINVAL, std::string("sweep_context: ") + why);
    if (target4->proj != COREG_PROJ_TAN || small->proj != COREG_PROJ_TAN)
        return fail(h, COREG_EINVAL, "sweep_context: SPICE headers must be HPLN-TAN / HPLT-TAN");
    RETCHK(check_order(h, order));
    // odd orders: scipy's first tap is floor(c), and every SPICE sample of this near-identity map sits within wcslib's
    // noise of an integer -- the tap set of EVERY sample would be noise-decided
    if (order & 1) return fail(h, COREG_ENOTIMPL, "sweep_context: odd reprojection orders are not implemented");
    if (method != COREG_METHOD_CORRELATION && method != COREG_METHOD_RESIDUS && method != COREG_METHOD_RESIDUS_MASKED)
        return fail(h, COREG_EINVAL, "sweep_context: unknown method");
    if (sem != COREG_CDELT_INTENDED && sem != COREG_CDELT_REFERENCE)
        return fail(h, COREG_EINVAL, "sweep_context: unknown cdelt semantics");
    const int gW = small->naxis1, gH = small->naxis2;
    if (gW != h->sW || gH != h->sH)
        return fail(h, COREG_EINVAL, "sweep_context: the SPICE image does not have the shape of its header");
    LagDims d;
    RETCHK(check_lags(h, lags, &d, lag_begin, lag_end));
    for (int i = 0; i < gW; ++i)
        if (col_frame[i] < 0 || col_frame[i] >= c->n) return fail(h, COREG_EINVAL, "sweep_context: col_frame out of range");
    const long long n_out = lag_end - lag_begin;
    if (n_out > 0 && !corr_out) return fail(h, COREG_EINVAL, "sweep_context: corr_out is null");
    RETCHK(bind_device(h));
    h->stats_pending = false;  // (as begin_sweep: the timings of an uncollected device-output sweep are dropped)
    reset_stats(h, (long long)gW * gH, n_out);
    h->stats.n_active_points = (long long)gW * gH;
    // re-evaluated lag-points of THIS sweep (coreg_last_visit_counts "refined_lag_points"), summed over its launches
    HIPCHK(h->counters.reserve(8 * sizeof(long long)));
    HIPCHK(hipMemsetAsync(h->counters.p, 0, 8 * sizeof(long long), h->stream));
    HIPCHK(h->counts.reserve((size_t)std::max<long long>(n_out, 1) * sizeof(double)));
    h->counts_n = n_out;
    if (n_out == 0) return COREG_OK;
    double* const counts = h->counts.as<double>();  // (every lag-point of the slice is finalised below: no NaN fill)

    HIPCHK(c->mean.reserve(2 * sizeof(double)));
    if (!c->have_pivot) {
        const long long nf = (long long)c->n * c->W * c->H;
        HIPCHK(buffer_mean(h, c->frames.p, c->f32, nf, c->mean.as<double>(), h->stream));
        HIPCHK(hipMemcpyAsync(&c->pivot, c->mean.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!std::isfinite(c->pivot)) c->pivot = 0.0;
        c->have_pivot = true;
    }
    double pivots[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(pivots, h->pivots.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double pb = std::isfinite(pivots[1]) ? pivots[1] : 0.0;

    double* out_dev = corr_out;
    if (!out_on_device) {
        HIPCHK(c->out_tmp.reserve((size_t)n_out * sizeof(double)));
        out_dev = c->out_tmp.as<double>();
    }
    HIPCHK(c->col_frame.reserve((size_t)gW * sizeof(int)));
    HIPCHK(hipMemcpyAsync(c->col_frame.p, col_frame, (size_t)gW * sizeof(int), hipMemcpyHostToDevice, h->stream));

    const int n_groups = (gW + kCtxCols - 1) / kCtxCols;
    const int ne = 2 * (gW + gH);
    std::vector<double> hc, hs;
    std::vector<unsigned char> ed;
    std::vector<long long> oi;
    float kernel_ms = 0.f;
    int launches = 0;
    for (long long b0 = lag_begin; b0 < lag_end; b0 += kCtxBatch) {
        const long long ns_ = std::min(kCtxBatch, lag_end - b0);
        hc.resize((size_t)ns_ * c->n * 9);
        hs.resize((size_t)ns_ * 9);
        ed.resize((size_t)ns_ * ne);
        oi.resize((size_t)ns_);
        for (long long s = 0; s < ns_; ++s) oi[s] = b0 + s;
        // the plan on the host: a few microseconds per (frame, lag) homography and per wcslib border evaluation
        parallel_for(ns_, 16, 32, [&](long long s0, long long s1) {
            context_plan_range(*c, *target4, *small, *lags, d, sem, b0, s0, s1, h->sW, h->sH, hc.data(), hs.data(),
                               ed.data());
        });
        HIPCHK(hipStreamSynchronize(h->stream));  // (the previous launch's plan buffers)
        HIPCHK(c->h_ctx.reserve(hc.size() * sizeof(double)));
        HIPCHK(c->h_sp.reserve(hs.size() * sizeof(double)));
        HIPCHK(c->edge.reserve(ed.size()));
        HIPCHK(c->out_index.reserve(oi.size() * sizeof(long long)));
        HIPCHK(c->partials.reserve((size_t)n_groups * kNumSums * ns_ * sizeof(double)));
        HIPCHK(c->flags.reserve((size_t)ns_ * sizeof(int)));
        HIPCHK(c->slot_pivots.reserve((size_t)2 * ns_ * sizeof(double)));
        HIPCHK(c->list.reserve((size_t)ns_ * sizeof(int)));
        HIPCHK(c->head.reserve(4 * sizeof(int)));
        HIPCHK(hipMemcpyAsync(c->h_ctx.p, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(c->h_sp.p, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(c->edge.p, ed.data(), ed.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(c->out_index.p, oi.data(), oi.size() * sizeof(long long), hipMemcpyHostToDevice,
                              h->stream));
        HIPCHK(hipMemsetAsync(c->head.p, 0, 4 * sizeof(int), h->stream));

        ContextArgs a = {};
        a.frames = c->frames.p;
        a.frames_f32 = c->f32 ? 1 : 0;
        a.fW = c->W;
        a.fH = c->H;
        a.col_frame = c->col_frame.as<int>();
        a.n_frames = c->n;
        a.small = h->small.p;
        a.small_f32 = h->small_f32 ? 1 : 0;
        a.sW = h->sW;
        a.sH = h->sH;
        a.order = order;
        a.gW = gW;
        a.gH = gH;
        a.h_ctx = c->h_ctx.as<double>();
        a.h_sp = c->h_sp.as<double>();
        a.edge = c->edge.as<unsigned char>();
        a.has_min = has_min ? 1 : 0;
        a.has_max = has_max ? 1 : 0;
        a.vmin = (float)vmin;  // (NumPy compares a float32 array with a Python float in float32)
        a.vmax = (float)vmax;
        a.residus = method == COREG_METHOD_RESIDUS_MASKED ? 2 : (method == COREG_METHOD_RESIDUS ? 1 : 0);
        a.n_slots = ns_;
        a.pa = a.residus ? 0.0 : c->pivot;
        a.pb = a.residus ? 0.0 : pb;
        a.partials = c->partials.as<double>();
        const dim3 grid((unsigned)n_groups, (unsigned)((ns_ + kCtxLags - 1) / kCtxLags));
        HIPCHK(hipEventRecord(c->ev_a, h->stream));
        context_types(c->f32, h->small_f32, [&](auto frame, auto spice) {
            hipLaunchKernelGGL((k_context_sweep<decltype(frame), decltype(spice)>), grid, dim3(kCtxThreads), 0, h->stream, a);
        });
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev_b, h->stream));
        ++launches;
        if (a.residus) {
            hipLaunchKernelGGL(k_finalize_context_residus, dim3((unsigned)((ns_ + 255) / 256)), dim3(256), 0, h->stream,
                               a.partials, n_groups, ns_, lag_begin, c->out_index.as<long long>(), out_dev,
                               a.residus == 2 ? 1 : 0, counts);
            HIPCHK(hipGetLastError());
        } else {
            FinalizeArgs f = {};
            f.partials = a.partials;
            f.n_groups = n_groups;
            f.n_slots = ns_;
            f.out_index = c->out_index.as<long long>();
            f.lag_begin = lag_begin;
            f.out = out_dev;
            f.counts = counts;
            f.part_stride = ns_;
            f.refine_count = h->counters.as<long long>();
            RefineArgs& r = f.refine;
            r.enabled = h->opt_refine ? 1 : 0;  // (options "refine", "refine_cond_log10")
            r.cond = std::pow(10.0, (double)h->opt_refine_cond_log10);
            r.flags = c->flags.as<int>();
            r.slot_pivots = c->slot_pivots.as<double>();
            r.list = c->list.as<int>();
            r.head = c->head.as<int>();
            r.out_index = f.out_index;
            r.lag_begin = lag_begin;
            r.out = out_dev;
            r.counts = counts;
            launch_finalize(h, f);
            if (r.enabled) {
                hipLaunchKernelGGL(k_refine_list, dim3(1), dim3(kListThreads), 0, h->stream, r, ns_, h->counters.as<long long>());
                context_types(c->f32, h->small_f32, [&](auto frame, auto spice) {
                    hipLaunchKernelGGL((k_refine_context<decltype(frame), decltype(spice)>), dim3(256), dim3(kCtxThreads), 0,
                                       h->stream, a, r);
                });
            }
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventSynchronize(c->ev_b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
        kernel_ms += ms;
    }
    if (!out_on_device)
        HIPCHK(hipMemcpyAsync(corr_out, out_dev, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stats.sweep_kernel_ms = kernel_ms;
    h->stats.n_sweep_launches = launches;
    return COREG_OK;
}

}  // namespace
