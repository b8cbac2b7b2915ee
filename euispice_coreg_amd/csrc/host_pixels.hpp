// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the integer pixel-lag sweep
// of pxlshift.AlignmentPixels -- per-handle state (PixelsState, freed with the handle that owns it),
// uploads, the displacement of the large image, the
// sub-resolved box, the rotation planes and the sweep itself (kernels: csrc/kernels_pixels.hpp).  A sweep is four steps
// (pixels_sweep_run): the plan -- every check of the request, groups, band, grid and blob layout, csrc/pixels_plan.hpp, no
// GPU work --, pixels_prepare (buffers, blob, box, rotation planes: the same for every score), the passes of one score
// (pixels_run_sums / _lct / _mi) and pixels_finish (the cube back, the record of what the sweep left).
#pragma once

// what the last sweep left in `counts` (and, apodized, in `weights`): nothing once an image has changed
enum PixLast { PIX_LAST_NONE = 0, PIX_LAST_UNTILED, PIX_LAST_TILED, PIX_LAST_APODIZED };

struct PixelsState {
    DevBuf large, large_tmp, small, box, planes, sums, plan, corr, counts, weights;
    int lW = 0, lH = 0, sW = 0, sH = 0;
    int bW = 0, bH = 0, n_rot = 0;  // what the last sweep left in `box` / `planes`
    PixLast last = PIX_LAST_NONE;   // ... and in `counts` / `weights`: its kind and
    long long last_n_out = 0;       //     its entries (lags, or tiles x lags)
    void forget_last() {
        last = PIX_LAST_NONE;
        last_n_out = 0;
    }
    Event ev[4];
    bool timed = false;
    // coreg_pixels_destretch: buffers, events and time of its own (the sweep's images, counts and events are not touched)
    DevBuf ds_src, ds_dst, ds_disp, ds_nodes;
    Event ds_ev[2];
    bool ds_timed = false;
    // coreg_pixels_set_bins: the edge lists of COREG_METHOD_MUTUAL_INFORMATION, kept until set again
    std::vector<double> edges_small, edges_large;
    // the dynamic LDS each k_pixels_mi instantiation ([tiled][wide]) has been allowed on this handle's device so far
    size_t mi_lds[2][2] = {{0, 0}, {0, 0}};
};

static PixelsState* pixels_state(coreg_handle* h, bool create) {
    if (!h->pix && create) h->pix.reset(new (std::nothrow) PixelsState());
    return h->pix.get();
}

static int pixels_upload(coreg_handle* h, DevBuf& buf, const void* img, int dtype, int32_t ny, int32_t nx, int* W, int* H) {
    if (!img || ny < 1 || nx < 1) return fail(h, COREG_EINVAL, "pixels: null image or empty shape");
    if (dtype != COREG_F32 && dtype != COREG_F64) return fail(h, COREG_EINVAL, "pixels: dtype must be COREG_F32 or COREG_F64");
    if (too_many(ny, nx)) return fail(h, COREG_EINVAL, "pixels: image too large");
    RETCHK(bind_device(h));
    const size_t n = (size_t)ny * nx;
    HIPCHK(buf.reserve(n * sizeof(double)));
    std::vector<double> conv;
    const void* src = img;
    if (dtype == COREG_F32) {
        conv.resize(n);
        const float* f = (const float*)img;
        for (size_t q = 0; q < n; ++q) conv[q] = (double)f[q];
        src = conv.data();
    }
    HIPCHK(hipMemcpyAsync(buf.p, src, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's / the converted pixels are free again)
    *W = nx;
    *H = ny;
    return COREG_OK;
}

static int pixels_resample(coreg_handle* h, int mode, const PixResample& a) {
    const long long n = (long long)a.dW * a.dH;
    const int nb = (int)std::min<long long>((n + kPixThreads - 1) / kPixThreads, 65535);
    if (mode == PIX_AFFINE)
        hipLaunchKernelGGL(k_pixels_resample<PIX_AFFINE>, dim3(nb), dim3(kPixThreads), 0, h->stream, a);
    else
        hipLaunchKernelGGL(k_pixels_resample<PIX_POLAR>, dim3(nb), dim3(kPixThreads), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

int pixels_set_large(coreg_handle* h, const void* img, int dtype, int32_t ny, int32_t nx) {
    PixelsState* st = pixels_state(h, true);
    if (!st) return fail(h, COREG_ENOMEM, "pixels: out of memory");
    st->bW = st->bH = 0;  // (the box of the last sweep is no longer this image's)
    st->forget_last();
    return pixels_upload(h, st->large, img, dtype, ny, nx, &st->lW, &st->lH);
}

int pixels_set_small(coreg_handle* h, const void* img, int dtype, int32_t ny, int32_t nx) {
    PixelsState* st = pixels_state(h, true);
    if (!st) return fail(h, COREG_ENOMEM, "pixels: out of memory");
    st->n_rot = 0;
    st->forget_last();
    return pixels_upload(h, st->small, img, dtype, ny, nx, &st->sW, &st->sH);
}

// alignment_pixels.py:86-107: an identity pass, then the pass at (x + dx, y + dy); fill -32762 -> NaN after each
int pixels_shift_large(coreg_handle* h, double dx, double dy) {
    PixelsState* st = pixels_state(h, false);
    if (!st || !st->large.p) return fail(h, COREG_ESTATE, "pixels: the large image is not set");
    if (!(dx == dx) || !(dy == dy)) return fail(h, COREG_EINVAL, "pixels: the displacement is not a number");
    RETCHK(bind_device(h));
    st->bW = st->bH = 0;
    st->forget_last();
    const size_t n = (size_t)st->lW * st->lH;
    HIPCHK(st->large_tmp.reserve(n * sizeof(double)));
    PixResample a = {};
    a.sW = a.dW = st->lW;
    a.sH = a.dH = st->lH;
    a.ax = a.ay = 1.0;
    a.fill = -32762.0;
    a.src = st->large.as<double>();
    a.dst = st->large_tmp.as<double>();
    RETCHK(pixels_resample(h, PIX_AFFINE, a));
    a.src = st->large_tmp.as<double>();
    a.dst = st->large.as<double>();
    a.bx = dx;
    a.by = dy;
    return pixels_resample(h, PIX_AFFINE, a);
}

// NaN-aware smoothing (host_smooth.hpp) of the large (which = 0) or small (1) image, in place: both are float64 already
int pixels_smooth(coreg_handle* h, int which, const double* wy, int32_t n_wy, const double* wx, int32_t n_wx) {
    PixelsState* st = pixels_state(h, false);
    DevBuf* img = st ? (which ? &st->small : &st->large) : nullptr;
    if (!img || !img->p) return fail(h, COREG_ESTATE, which ? "pixels: the small image is not set" : "pixels: the large image is not set");
    const int W = which ? st->sW : st->lW, H = which ? st->sH : st->lH;
    const SmoothPlan p = smooth_plan(H, W, wy, n_wy, wx, n_wx);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);  // (a refused call changes nothing)
    RETCHK(bind_device(h));
    if (which) st->n_rot = 0;
    else st->bW = st->bH = 0;
    st->forget_last();
    return smooth_image(h, img->p, false, H, W, wy, n_wy, wx, n_wx, img->as<double>());
}

// median/MAD despiking (host_despike.hpp) of the large (which = 0) or small (1) image, in place as far as the caller sees:
// the buffer of the last pass changes places with the image's (both float64)
int pixels_despike(coreg_handle* h, int which, const coreg_despike_params* params, int64_t* n_flagged) {
    PixelsState* st = pixels_state(h, false);
    DevBuf* img = st ? (which ? &st->small : &st->large) : nullptr;
    if (!img || !img->p) return fail(h, COREG_ESTATE, which ? "pixels: the small image is not set" : "pixels: the large image is not set");
    const int W = which ? st->sW : st->lW, H = which ? st->sH : st->lH;
    const DespikePlan p = despike_plan(H, W, params);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);  // (a refused call changes nothing)
    RETCHK(bind_device(h));
    if (which) st->n_rot = 0;
    else st->bW = st->bH = 0;
    st->forget_last();
    DevBuf* done = nullptr;
    RETCHK(despike_image(h, img->p, false, H, W, params, DESPIKE_SLOT_IMAGE, &done));
    std::swap(*img, *done);
    if (n_flagged) RETCHK(despike_read_counts(h, DESPIKE_SLOT_IMAGE, params->n_iter, n_flagged));
    return COREG_OK;
}

// the edge lists of the mutual-information score (csrc/pixels_bins.hpp: 1 to 31 entries, finite, strictly increasing)
int pixels_set_bins(coreg_handle* h, const double* edges_small, int32_t n_small, const double* edges_large, int32_t n_large) {
    if (!bins_edges_ok(edges_small, n_small) || !bins_edges_ok(edges_large, n_large))
        return fail(h, COREG_EINVAL, "pixels: an edge list needs 1 to 31 finite, strictly increasing entries");
    PixelsState* st = pixels_state(h, true);
    if (!st) return fail(h, COREG_ENOMEM, "pixels: out of memory");
    st->edges_small.assign(edges_small, edges_small + n_small);
    st->edges_large.assign(edges_large, edges_large + n_large);
    return COREG_OK;
}

template <int PASS>
static void pixels_launch_pass(coreg_handle* h, const dim3& grid, const PixSweep& s, const PixTiles* t, const PixStep& step) {
    if (t)
        hipLaunchKernelGGL(k_pixels_sweep_tiles<PASS>, grid, dim3(kPixThreads), 0, h->stream, s, *t, step);
    else
        hipLaunchKernelGGL(k_pixels_sweep<PASS>, grid, dim3(kPixThreads), 0, h->stream, s);
}

// The histograms at 32 x 32 bins are 64 KiB of dynamic LDS beside the kernel's static 13.5 KiB: more than the 64 KiB a
// workgroup has on CDNA1-3.  gfx950 gives a workgroup up to 160 KiB; the kernel is allowed what it needs, once per
// instantiation and again only when a later sweep needs more (`allowed`: PixelsState::mi_lds).
static_assert((size_t)kPixG * kPixMaxBins * kPixMaxBins * sizeof(uint32_t) + 16 * 1024 <= 160 * 1024,
              "k_pixels_mi: histograms and staging must fit the 160 KiB of LDS of a gfx950 workgroup");

template <bool TILED, int THREADS>
static int pixels_launch_mi(coreg_handle* h, const dim3& grid, size_t dyn, size_t* allowed, const PixSweep& s, const PixTiles& t,
                            const PixBins& b, const PixStep& step) {
    if (dyn > *allowed) {
        HIPCHK(hipFuncSetAttribute((const void*)k_pixels_mi<TILED, THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        *allowed = dyn;
    }
    hipLaunchKernelGGL((k_pixels_mi<TILED, THREADS>), grid, dim3(THREADS), dyn, h->stream, s, t, b, step);
    return COREG_OK;
}

// What every score needs, from the reservations on (the record of the last sweep ends here): buffers, the plan blob on
// the device, the box, the rotation planes -- events 0 and 1 about the two resamples -- and the kernels' common arguments.
static int pixels_prepare(coreg_handle* h, PixelsState* st, const coreg_pixels_plan* pl, const PixPlan& p, const double* wy,
                          const double* wx, PixSweep* s) {
    const int w = st->sW, hh = st->sH;
    std::vector<unsigned char> blob(p.bytes);
    pixels_plan_write(p, pl, p.mi ? st->edges_small.data() : wy, p.mi ? st->edges_large.data() : wx, blob.data());
    HIPCHK(st->plan.reserve(blob.size()));
    HIPCHK(st->box.reserve((size_t)p.bW * p.bH * sizeof(double)));
    HIPCHK(st->planes.reserve((size_t)w * hh * pl->n_rot * sizeof(double)));
    if (!p.mi) HIPCHK(st->sums.reserve((size_t)p.n_out * (p.lct ? 7 : 6) * sizeof(double)));
    if (p.lct) HIPCHK(st->weights.reserve((size_t)p.n_out * sizeof(double)));
    HIPCHK(st->corr.reserve((size_t)p.n_out * sizeof(double)));
    HIPCHK(st->counts.reserve((size_t)p.n_out * sizeof(double)));
    st->forget_last();
    for (Event& e : st->ev)
        if (!e) HIPCHK(hipEventCreate(&e.e));
    st->timed = false;
    HIPCHK(hipMemcpyAsync(st->plan.p, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventRecord(st->ev[0], h->stream));

    // the part of the sub-resolved large image the lags can reach (alignment_pixels.py:126-143)
    PixResample a = {};
    a.src = st->large.as<double>();
    a.sW = st->lW;
    a.sH = st->lH;
    a.dst = st->box.as<double>();
    a.dW = p.bW;
    a.dH = p.bH;
    a.i0 = pl->l1 + p.min_dx;
    a.j0 = pl->l0 + p.min_dy;
    a.ax = pl->ratio1;
    a.ay = pl->ratio2;
    a.fill = -32768.0;
    RETCHK(pixels_resample(h, PIX_AFFINE, a));
    st->bW = p.bW;
    st->bH = p.bH;
    // rotation planes (alignment_pixels.py:72-81), each from the original
    for (int k = 0; k < pl->n_rot; ++k) {
        double* plane = st->planes.as<double>() + (size_t)k * w * hh;
        if (pl->lag_drot[k] == 0.0) {
            HIPCHK(hipMemcpyAsync(plane, st->small.p, (size_t)w * hh * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            continue;
        }
        PixResample r = {};
        r.src = st->small.as<double>();
        r.sW = r.dW = w;
        r.sH = r.dH = hh;
        r.dst = plane;
        r.xc = (double)pl->xc;
        r.yc = (double)pl->yc;
        r.drot = pl->lag_drot[k];
        r.fill = -32762.0;
        RETCHK(pixels_resample(h, PIX_POLAR, r));
    }
    st->n_rot = pl->n_rot;
    HIPCHK(hipEventRecord(st->ev[1], h->stream));

    *s = {};
    s->planes = st->planes.as<double>();
    s->box = st->box.as<double>();
    s->groups = pixels_plan_at<PixGroup>(st->plan.p, 0);
    s->lag_dx = pixels_plan_at<int>(st->plan.p, p.off_dx);
    s->lag_dy = pixels_plan_at<int>(st->plan.p, p.off_dy);
    s->w = w;
    s->h = hh;
    s->bW = p.bW;
    s->bH = p.bH;
    s->n_dx = pl->n_dx;
    s->n_dy = pl->n_dy;
    s->min_dx = p.min_dx;
    s->min_dy = p.min_dy;
    s->cw = p.cw;
    s->bh = p.bh;
    return COREG_OK;
}

// The passes of one score.  (The three functions stand in the order in which the sweep first named their kernels -- mutual
// information, apodized, sums: the compiler emits the kernels in that order, and the device code stays as it was.)
// Mutual information, one pass: histograms, score and counts (csrc/kernels_pixels_mi.hpp); the last two events bracket nothing
static int pixels_run_mi(coreg_handle* h, PixelsState* st, const coreg_pixels_plan* pl, const PixPlan& p, const PixSweep& s) {
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    PixBins b = {};
    b.edges_small = pixels_plan_at<double>(st->plan.p, p.off_a);
    b.edges_large = pixels_plan_at<double>(st->plan.p, p.off_b);
    b.n_small = p.n_a;
    b.n_large = p.n_b;
    b.corr = st->corr.as<double>();
    b.counts = st->counts.as<double>();
    b.n_rot = pl->n_rot;
    const size_t dyn = (size_t)kPixG * (b.n_small + 1) * (b.n_large + 1) * sizeof(uint32_t);
    const bool wide = dyn > kPixMiWideBytes;
    size_t* allowed = &st->mi_lds[p.tiled ? 1 : 0][wide ? 1 : 0];
    RETCHK(p.tiled ? (wide ? pixels_launch_mi<true, kPixMiThreadsWide>(h, grid, dyn, allowed, s, p.tl, b, p.ts)
                           : pixels_launch_mi<true, kPixMiThreads>(h, grid, dyn, allowed, s, p.tl, b, p.ts))
                   : (wide ? pixels_launch_mi<false, kPixMiThreadsWide>(h, grid, dyn, allowed, s, p.tl, b, p.ts)
                           : pixels_launch_mi<false, kPixMiThreads>(h, grid, dyn, allowed, s, p.tl, b, p.ts)));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], h->stream));
    HIPCHK(hipEventRecord(st->ev[3], h->stream));
    return COREG_OK;
}

// the apodized windows: four sums, then three (csrc/kernels_pixels_lct.hpp), and a finalize step of their own
static int pixels_run_lct(coreg_handle* h, PixelsState* st, const coreg_pixels_plan* pl, const PixPlan& p, PixSweep s) {
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    const PixWindow win = {pixels_plan_at<double>(st->plan.p, p.off_a), pixels_plan_at<double>(st->plan.p, p.off_b)};
    double* sums0 = st->sums.as<double>();
    double* lsums1 = sums0 + 4 * p.n_out;
    s.sums0 = nullptr;
    s.sums = sums0;
    hipLaunchKernelGGL(k_pixels_lct<0>, grid, dim3(kPixThreads), 0, h->stream, s, p.tl, p.ts, win);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], h->stream));
    s.sums0 = sums0;
    s.sums = lsums1;
    hipLaunchKernelGGL(k_pixels_lct<1>, grid, dim3(kPixThreads), 0, h->stream, s, p.tl, p.ts, win);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[3], h->stream));
    hipLaunchKernelGGL(k_pixels_lct_finalize, dim3(p.fin_grid[0], p.fin_grid[1]), dim3(kPixThreads), 0, h->stream,
                       (const double*)sums0, (const double*)lsums1, pl->n_dx, pl->n_dy, pl->n_rot, st->corr.as<double>(),
                       st->counts.as<double>(), st->weights.as<double>());
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

// Pearson or residus_masked: the two passes, events 2 and 3 behind them, and k_pixels_finalize
static int pixels_run_sums(coreg_handle* h, PixelsState* st, const coreg_pixels_plan* pl, const PixPlan& p, PixSweep s) {
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    const PixTiles* t = p.tiled ? &p.tl : nullptr;
    double* sums0 = st->sums.as<double>();
    double* sums1 = sums0 + 3 * p.n_out;
    s.sums0 = nullptr;
    s.sums = sums0;
    if (p.resid)
        pixels_launch_pass<kPixR0>(h, grid, s, t, p.ts);
    else
        pixels_launch_pass<0>(h, grid, s, t, p.ts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], h->stream));
    s.sums0 = sums0;
    s.sums = sums1;
    if (p.resid)
        pixels_launch_pass<kPixR1>(h, grid, s, t, p.ts);
    else
        pixels_launch_pass<1>(h, grid, s, t, p.ts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[3], h->stream));
    hipLaunchKernelGGL(k_pixels_finalize, dim3(p.fin_grid[0], p.fin_grid[1]), dim3(kPixThreads), 0, h->stream,
                       (const double*)sums0, (const double*)sums1, pl->n_dx, pl->n_dy, pl->n_rot, (int)p.resid,
                       st->corr.as<double>(), st->counts.as<double>());
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

// the one tail: the cube back, and what this sweep left for the getters
static int pixels_finish(coreg_handle* h, PixelsState* st, const PixPlan& p, double* corr_out) {
    HIPCHK(hipMemcpyAsync(corr_out, st->corr.p, (size_t)p.n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    st->timed = true;
    st->last = !p.tiled ? PIX_LAST_UNTILED : p.lct ? PIX_LAST_APODIZED : PIX_LAST_TILED;
    st->last_n_out = p.n_out;
    return COREG_OK;
}

// The untiled sweep (tile == nullptr) and the tiled one, any score (the arguments: PixRequest, csrc/pixels_plan.hpp).  A
// request the plan refuses changes nothing of the handle's state but its error text.
static int pixels_sweep_run(coreg_handle* h, const coreg_pixels_plan* pl, int method, const int32_t* tile, const int32_t* step,
                            const double* wy, const double* wx, double* corr_out) {
    PixelsState* st = pixels_state(h, false);
    PixHave have = {};
    if (st)
        have = {st->large.p != nullptr, st->small.p != nullptr, st->sW, st->sH, (int)st->edges_small.size(),
                (int)st->edges_large.size()};
    const PixPlan p = pixels_plan(PixRequest{pl, method, tile, step, wy, wx, corr_out}, have);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);
    RETCHK(bind_device(h));
    PixSweep s;
    RETCHK(pixels_prepare(h, st, pl, p, wy, wx, &s));
    RETCHK(p.mi ? pixels_run_mi(h, st, pl, p, s) : p.lct ? pixels_run_lct(h, st, pl, p, s) : pixels_run_sums(h, st, pl, p, s));
    return pixels_finish(h, st, p, corr_out);
}

int pixels_sweep(coreg_handle* h, const coreg_pixels_plan* pl, int method, double* corr_out) {
    return pixels_sweep_run(h, pl, method, nullptr, nullptr, nullptr, nullptr, corr_out);
}

// out[n_ty][n_tx][n_dx][n_dy][n_rot]: the cube of every tile of tile_ny x tile_nx small-image pixels (the last ones ragged)
int pixels_sweep_tiles(coreg_handle* h, const coreg_pixels_plan* pl, int method, int32_t tile_ny, int32_t tile_nx, double* out) {
    const int32_t tile[2] = {tile_ny, tile_nx};
    return pixels_sweep_run(h, pl, method, tile, nullptr, nullptr, nullptr, out);
}

// The same on a grid of windows: their origins step_ny x step_nx apart (1 <= step <= tile: they overlap, n_ty = 1 when
// h <= tile_ny, else ceil((h - tile_ny) / step_ny) + 1), and, with the tables wy[tile_ny], wx[tile_nx], every pixel weighted by
// wy[row in the window] * wx[column in the window] (the correlation only)
int pixels_sweep_windows(coreg_handle* h, const coreg_pixels_plan* pl, int method, int32_t tile_ny, int32_t tile_nx,
                         int32_t step_ny, int32_t step_nx, const double* wy, const double* wx, double* out) {
    const int32_t tile[2] = {tile_ny, tile_nx}, step[2] = {step_ny, step_nx};
    return pixels_sweep_run(h, pl, method, tile, step, wy, wx, out);
}

int pixels_last_timing(coreg_handle* h, double* ms) {
    PixelsState* st = pixels_state(h, false);
    if (!st || !st->timed) return fail(h, COREG_ESTATE, "pixels: no sweep has run");
    if (!ms) return fail(h, COREG_EINVAL, "pixels: null pointer");
    RETCHK(bind_device(h));
    for (int k = 0; k < 3; ++k) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, st->ev[k], st->ev[k + 1]));
        ms[k] = (double)t;
    }
    return COREG_OK;
}

static int pixels_read(coreg_handle* h, const void* dev, size_t n, double* out) {
    if (!out) return fail(h, COREG_EINVAL, "pixels: null pointer");
    RETCHK(bind_device(h));
    HIPCHK(hipMemcpyAsync(out, dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

// the large (which = 0) or small (1) image as it stands: [ny][nx] float64
int pixels_get_image(coreg_handle* h, int which, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (which != 0 && which != 1) return fail(h, COREG_EINVAL, "pixels: which must be 0 (large) or 1 (small)");
    DevBuf* img = st ? (which ? &st->small : &st->large) : nullptr;
    if (!img || !img->p) return fail(h, COREG_ESTATE, "pixels: that image is not set");
    return pixels_read(h, img->p, which ? (size_t)st->sW * st->sH : (size_t)st->lW * st->lH, out);
}

int pixels_get_large_box(coreg_handle* h, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (!st || st->bW < 1) return fail(h, COREG_ESTATE, "pixels: no sweep has run");
    return pixels_read(h, st->box.p, (size_t)st->bW * st->bH, out);
}

int pixels_get_rotated(coreg_handle* h, int32_t k, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (!st || st->n_rot < 1) return fail(h, COREG_ESTATE, "pixels: no sweep has run");
    if (k < 0 || k >= st->n_rot) return fail(h, COREG_EINVAL, "pixels: rotation index out of range");
    const size_t n = (size_t)st->sW * st->sH;
    return pixels_read(h, st->planes.as<double>() + n * k, n, out);
}

// per-lag sample counts of the last sweep, laid out like its cube
int pixels_last_counts(coreg_handle* h, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (!st || st->last != PIX_LAST_UNTILED) return fail(h, COREG_ESTATE, "pixels: no untiled sweep has run since the images were set");
    return pixels_read(h, st->counts.p, (size_t)st->last_n_out, out);
}

// the same of the last tiled sweep: [n_ty][n_tx][n_dx][n_dy][n_rot]
int pixels_last_tile_counts(coreg_handle* h, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (!st || (st->last != PIX_LAST_TILED && st->last != PIX_LAST_APODIZED)) return fail(h, COREG_ESTATE, "pixels: no tiled sweep has run since the images were set");
    return pixels_read(h, st->counts.p, (size_t)st->last_n_out, out);
}

// the sums of weights W of the last tiled sweep when it was apodized, laid out like its cubes
int pixels_last_tile_weights(coreg_handle* h, double* out) {
    PixelsState* st = pixels_state(h, false);
    if (!st || st->last != PIX_LAST_APODIZED)
        return fail(h, COREG_ESTATE, "pixels: the last sweep since the images were set was not an apodized one");
    return pixels_read(h, st->weights.p, (size_t)st->last_n_out, out);
}

// The destretch of a cube [n_planes][ny][nx] by a local shift field (csrc/pixels_field.hpp, k_pixels_destretch): every
// argument is checked before any GPU work; the cube goes up as stored and comes back in its own type.
int pixels_destretch(coreg_handle* h, const void* cube, int dtype, int32_t n_planes, int32_t ny, int32_t nx,
                     const coreg_pixels_field* f, void* out, double* displacement) {
    if (!cube || !out || !f || !f->ys || !f->xs || !f->u || !f->v) return fail(h, COREG_EINVAL, "destretch: null pointer");
    if (dtype != COREG_F32 && dtype != COREG_F64) return fail(h, COREG_EINVAL, "destretch: dtype must be COREG_F32 or COREG_F64");
    if (n_planes < 1 || ny < 1 || nx < 1) return fail(h, COREG_EINVAL, "destretch: empty cube");
    if (too_many(ny, nx) || too_many((long long)ny * nx, n_planes))
        return fail(h, COREG_EINVAL, "destretch: more than 2^31 - 1 elements (cut the cube along its planes)");
    if (f->interpolation != PIX_FIELD_BILINEAR && f->interpolation != PIX_FIELD_NEAREST)
        return fail(h, COREG_EINVAL, "destretch: unknown interpolation (0 bilinear, 1 nearest)");
    if (f->n_ty < 1 || f->n_tx < 1 || f->tile_ny < 1 || f->tile_nx < 1 || too_many(f->n_ty, f->n_tx))
        return fail(h, COREG_EINVAL, "destretch: the field needs at least one node per axis and a positive tile shape");
    if (!std::isfinite(f->row_offset) || !std::isfinite(f->col_offset))
        return fail(h, COREG_EINVAL, "destretch: an offset is not finite");
    const int naxis[2] = {f->n_ty, f->n_tx};
    const double* axis[2] = {f->ys, f->xs};
    for (int a = 0; a < 2; ++a)
        for (int k = 0; k < naxis[a]; ++k)
            if (!std::isfinite(axis[a][k]) || (k > 0 && !(axis[a][k] > axis[a][k - 1])))
                return fail(h, COREG_EINVAL, "destretch: node coordinates must be finite and strictly increasing");
    const size_t n_nodes = (size_t)f->n_ty * f->n_tx;
    for (size_t k = 0; k < n_nodes; ++k)
        if (!std::isfinite(f->u[k]) || !std::isfinite(f->v[k])) return fail(h, COREG_EINVAL, "destretch: a node is not finite");
    PixelsState* st = pixels_state(h, true);
    if (!st) return fail(h, COREG_ENOMEM, "pixels: out of memory");
    RETCHK(bind_device(h));
    const size_t n_pix = (size_t)ny * nx, n = n_pix * (size_t)n_planes;
    const size_t bytes = n * (dtype == COREG_F32 ? sizeof(float) : sizeof(double));
    // the nodes on the device: ys, xs, u, v one after the other
    std::vector<double> nodes;
    nodes.reserve(f->n_ty + f->n_tx + 2 * n_nodes);
    nodes.insert(nodes.end(), f->ys, f->ys + f->n_ty);
    nodes.insert(nodes.end(), f->xs, f->xs + f->n_tx);
    nodes.insert(nodes.end(), f->u, f->u + n_nodes);
    nodes.insert(nodes.end(), f->v, f->v + n_nodes);
    HIPCHK(st->ds_nodes.reserve(nodes.size() * sizeof(double)));
    HIPCHK(st->ds_src.reserve(bytes));
    HIPCHK(st->ds_dst.reserve(bytes));
    if (displacement) HIPCHK(st->ds_disp.reserve(2 * n_pix * sizeof(double)));
    for (Event& e : st->ds_ev)
        if (!e) HIPCHK(hipEventCreate(&e.e));
    st->ds_timed = false;
    HIPCHK(hipMemcpyAsync(st->ds_nodes.p, nodes.data(), nodes.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->ds_src.p, cube, bytes, hipMemcpyHostToDevice, h->stream));
    PixDestretch a = {};
    a.src = st->ds_src.p;
    a.dst = st->ds_dst.p;
    a.disp = displacement ? st->ds_disp.as<double>() : nullptr;
    a.f.n_ty = f->n_ty;
    a.f.n_tx = f->n_tx;
    a.f.th = f->tile_ny;
    a.f.tw = f->tile_nx;
    a.f.interp = f->interpolation;
    a.f.ys = st->ds_nodes.as<double>();
    a.f.xs = a.f.ys + f->n_ty;
    a.f.u = a.f.xs + f->n_tx;
    a.f.v = a.f.u + n_nodes;
    a.f.row_offset = f->row_offset;
    a.f.col_offset = f->col_offset;
    a.nx = nx;
    a.ny = ny;
    a.n_planes = n_planes;
    const long long chunks = ((long long)n_planes + kPixDsPlanes - 1) / kPixDsPlanes;
    const dim3 grid((unsigned)((n_pix + kPixThreads - 1) / kPixThreads), (unsigned)std::min<long long>(chunks, 65535));
    HIPCHK(hipEventRecord(st->ds_ev[0], h->stream));
    if (dtype == COREG_F32)
        hipLaunchKernelGGL(k_pixels_destretch<float>, grid, dim3(kPixThreads), 0, h->stream, a);
    else
        hipLaunchKernelGGL(k_pixels_destretch<double>, grid, dim3(kPixThreads), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ds_ev[1], h->stream));
    HIPCHK(hipMemcpyAsync(out, st->ds_dst.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (displacement)
        HIPCHK(hipMemcpyAsync(displacement, st->ds_disp.p, 2 * n_pix * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    st->ds_timed = true;
    return COREG_OK;
}

int pixels_destretch_last_ms(coreg_handle* h, double* ms) {
    PixelsState* st = pixels_state(h, false);
    if (!st || !st->ds_timed) return fail(h, COREG_ESTATE, "destretch: no destretch has run");
    if (!ms) return fail(h, COREG_EINVAL, "destretch: null pointer");
    RETCHK(bind_device(h));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, st->ds_ev[0], st->ds_ev[1]));
    *ms = (double)t;
    return COREG_OK;
}
