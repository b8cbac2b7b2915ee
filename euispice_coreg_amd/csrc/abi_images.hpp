// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): C ABI: image to align, thresholds, reference on the grid / prepared on the GPU, resampling.
#pragma once
extern "C" {
// the checks every image hand-over shares: a pointer, a shape, fewer than 2^31 pixels
static int check_image(coreg_handle* h, const void* img, int32_t ny, int32_t nx, const char* who) {
    if (!img || ny < 1 || nx < 1 || too_many(ny, nx))
        return fail(h, COREG_EINVAL, std::string(who) + ": bad image (null pointer, empty, or more than 2^31 - 1 pixels)");
    return COREG_OK;
}
static bool is_dtype(int dtype) { return dtype == COREG_F32 || dtype == COREG_F64; }

// The image to align is on the device (h->small): record shape and type and enqueue its pivot on `s`, the stream that
// brought it; when that is the upload stream, leave the event the first reader of the image joins on (join_small).
static int adopt_small(coreg_handle* h, int32_t ny, int32_t nx, bool f32, hipStream_t s) {
    h->sW = nx;
    h->sH = ny;
    h->small_f32 = f32;
    HIPCHK(buffer_mean(h, h->small.p, f32, (long long)ny * nx, h->pivots.as<double>() + 1, s));
    return end_small_upload(h, s);
}

// Image to align from any source: `src` holds ny x nx pixels of format `fmt` in memory of `kind`, or (SRC_TILED) is a
// coreg_fits_tiled.  Pageable float32 pixels -- native, or BITPIX = -32 without scaling (what an EUI level-2 file without
// tile compression holds) -- go up on the upload stream, so that a reference preparation called next does not wait for
// them, and with "async_upload" from the handle's upload thread.  Everything else runs on the handle's stream.
static int set_small_from(coreg_handle* h, const void* src, const PixFmt& fmt, SrcKind kind, int32_t ny, int32_t nx) {
    RETCHK(check_image(h, src, ny, nx, "set_small"));
    const size_t n = (size_t)ny * nx;
    if (kind == SRC_HOST && (fmt.raw() ? fmt.swap_only() : fmt.f32)) {
        trace("set_small_f32: enter");
        RETCHK(bind_device(h));
        HIPCHK(h->small.reserve(n * sizeof(float)));
        hipStream_t s;
        RETCHK(begin_small_upload(h, &s));
        if (h->opt_async_upload && s != h->stream) {
            // the worker issues copies, byte swap and pivot and records ev_small itself; the caller's buffer must stay
            // valid until the next call that reads the image returns
            h->small_f32 = true;
            h->sW = nx;
            h->sH = ny;
            void* dev = h->small.p;
            const bool swap32 = fmt.raw();
            post_upload(h, [h, dev, src, n, swap32, s] { return upload_small_worker(h, dev, src, n, swap32, s); });
            h->small_pending = true;  // (join_small: waits for the worker to have issued everything, then for ev_small)
            trace("set_small_f32: handed to the upload thread");
            return COREG_OK;
        }
        // through pinned staging: the caller's buffer is free again on return, the copy itself is asynchronous
        RETCHK(staged_upload(h, h->small.p, src, n * sizeof(float), s));
        if (fmt.raw()) fits_swap32(h->small.p, n, s);
        RETCHK(adopt_small(h, ny, nx, true, s));
        trace("set_small_f32: issued");
        return COREG_OK;
    }
    RETCHK(bind_device(h));
    bool f32 = true;
    if (kind == SRC_TILED) {
        RETCHK(decode_tiled_device(h, (const coreg_fits_tiled*)src, h->small, &f32));
    } else if (fmt.raw()) {  // raw bytes up, decode on the GPU (an unscaled BITPIX = -32 is swapped where it lands)
        DevBuf& dst = fmt.swap_only() ? h->small : h->up_raw;
        HIPCHK(dst.reserve(n * fmt.elem()));
        RETCHK(copy_in(h, dst.p, src, n * fmt.elem(), kind));
        RETCHK(fits_decode(h, fmt, dst.p, n, h->small, &f32));
    } else if (fmt.f32) {  // page-locked or device memory: one asynchronous copy, no staging
        HIPCHK(h->small.reserve(n * sizeof(float)));
        RETCHK(copy_in(h, h->small.p, src, n * sizeof(float), kind));
    } else {
        RETCHK(upload_image(h, (const double*)src, n, h->small, &f32, kind));
    }
    return adopt_small(h, ny, nx, f32, h->stream);
}

int coreg_set_small(coreg_handle* h, const double* img, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    return set_small_from(h, img, PixFmt::native(false), SRC_HOST, ny, nx);
}

int coreg_set_small_f32(coreg_handle* h, const float* img, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    return set_small_from(h, img, PixFmt::native(true), SRC_HOST, ny, nx);
}

int coreg_set_small_from_device(coreg_handle* h, const void* dev_img, int dtype, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    if (!is_dtype(dtype)) return fail(h, COREG_EINVAL, "set_small: bad dtype");
    return set_small_from(h, dev_img, PixFmt::native(dtype == COREG_F32), SRC_DEVICE, ny, nx);
}

// image to align as the FITS data unit stores it (host memory): raw bytes up, decode on the GPU
int coreg_set_small_fits(coreg_handle* h, const coreg_fits_pixels* px, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    PixFmt fmt;
    RETCHK(check_fits(h, px, &fmt));
    return set_small_from(h, px->data, fmt, SRC_HOST, ny, nx);
}

int coreg_set_small_tiled(coreg_handle* h, const coreg_fits_tiled* t) {
    if (!h) return COREG_EINVAL;
    if (!t) return fail(h, COREG_EINVAL, "tiled image: null pointer");
    return set_small_from(h, t, PixFmt(), SRC_TILED, t->naxis2, t->naxis1);
}

int coreg_decode_tiled_host(const coreg_fits_tiled* t, void* out, int dtype, int32_t* tile_status) {
    if (check_tiled(t) || !out || (dtype != COREG_F32 && dtype != COREG_F64)) return COREG_EINVAL;
    if (dtype == COREG_F32 && t->zbitpix != -32) return COREG_EINVAL;
    coregrice::TileImage im;
    fill_tile_image(*t, &im);
    im.heap = (const unsigned char*)t->heap;
    im.tile_offset = t->tile_offset;
    im.tile_nbytes = t->tile_nbytes;
    im.zscale = t->zscale;
    im.zzero = t->zzero;
    im.randoms = host_randoms();
    im.out = out;
    im.out_dtype = dtype == COREG_F32 ? coregrice::OUT_F32 : coregrice::OUT_F64;
    const int nt = t->n_tiles;
    auto work = [&](int lo, int hi) {
        for (int k = lo; k < hi; ++k) {
            const int e = coregrice::decode_tile(im, k);
            if (tile_status) tile_status[k] = e;
        }
    };
    parallel_for(nt, (unsigned)std::min<long long>(12, (long long)t->naxis1 * t->naxis2 / (1 << 16)), 0, work);
    return COREG_OK;
}

int coreg_encode_tiled_host(const void* pixels, int dtype, int ny, int nx, int tile_x, int tile_y, int bytepix,
                            int blocksize, int quantize, int dither0, double scale, unsigned char* heap,
                            long long heap_cap, int32_t* tile_nbytes, int64_t* tile_offset, double* zscale, double* zzero,
                            long long* heap_used) {
    if (!pixels || !heap || !tile_nbytes || !tile_offset || !heap_used || ny <= 0 || nx <= 0 || tile_x <= 0 || tile_y <= 0)
        return COREG_EINVAL;
    if (blocksize <= 0 || blocksize > 1024 || (bytepix != 1 && bytepix != 2 && bytepix != 4)) return COREG_EINVAL;
    const bool is_float = dtype == COREG_F32 || dtype == COREG_F64;
    if (is_float) {
        if (quantize < coregrice::Q_NO_DITHER || quantize > coregrice::Q_DITHER_2 || !(scale > 0) || !std::isfinite(scale) ||
            !zscale || !zzero || bytepix != 4)
            return COREG_EINVAL;
    } else if (dtype != COREG_I32) {
        return COREG_EINVAL;  // integer images: the stored integers as int32, whatever BYTEPIX
    }
    coregrice::TileImage t{};
    t.naxis1 = nx;
    t.naxis2 = ny;
    t.ztile1 = tile_x;
    t.ztile2 = tile_y;
    t.dither0 = dither0;
    const int ntx = (nx + tile_x - 1) / tile_x, nty = (ny + tile_y - 1) / tile_y;
    std::vector<int32_t> q((size_t)tile_x * tile_y);
    long long used = 0;
    for (int n = 0; n < ntx * nty; ++n) {
        const coregrice::TileBox b = coregrice::tile_box(t, n);
        const int npx = b.tw * b.th;
        if (is_float) {
            const int iseed = coregrice::dither_seed(t, n);
            const int e = dtype == COREG_F32
                              ? coregrice::quantize_tile((const float*)pixels, nx, b, quantize, iseed, host_randoms(), scale,
                                                         q.data(), &zzero[n])
                              : coregrice::quantize_tile((const double*)pixels, nx, b, quantize, iseed, host_randoms(), scale,
                                                         q.data(), &zzero[n]);
            if (e) return COREG_EINVAL;  // (the tile's range does not fit 32-bit integers at this scale)
            zscale[n] = scale;
        } else {
            const int32_t* src = (const int32_t*)pixels;
            for (int y = 0; y < b.th; ++y)
                std::memcpy(q.data() + (size_t)y * b.tw, src + (size_t)(b.y0 + y) * nx + b.x0, (size_t)b.tw * 4);
        }
        const int64_t len = coregrice::rice_encode_tile(q.data(), npx, blocksize, bytepix, heap + used, heap_cap - used);
        if (len < 0) return COREG_ENOMEM;
        tile_offset[n] = used;
        tile_nbytes[n] = (int32_t)len;
        used += len;
    }
    *heap_used = used;
    return COREG_OK;
}

int coreg_threshold_small(coreg_handle* h, int has_min, double vmin, int has_max, double vmax, long long* n_finite) {
    if (!h) return COREG_EINVAL;
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    RETCHK(bind_device(h));
    const long long n = (long long)h->sW * h->sH;
    if (has_min || has_max) {
        const int nb = (int)std::min<long long>((n + 255) / 256, 2048);
        if (h->small_f32)
            hipLaunchKernelGGL((k_threshold<float>), dim3(nb), dim3(256), 0, h->stream, h->small.as<float>(), n, has_min,
                               vmin, has_max, vmax);
        else
            hipLaunchKernelGGL((k_threshold<double>), dim3(nb), dim3(256), 0, h->stream, h->small.as<double>(), n, has_min,
                               vmin, has_max, vmax);
        HIPCHK(hipGetLastError());
    }
    // pivot = mean of what is left (same value as uploading a host-thresholded image)
    HIPCHK(buffer_mean(h, h->small.p, h->small_f32, n, h->pivots.as<double>() + 1, h->stream));
    if (n_finite) {
        long long cnt[256];
        HIPCHK(hipMemcpyAsync(cnt, h->red_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        long long c = 0;
        for (int i = 0; i < 256; ++i) c += cnt[i];
        *n_finite = c;
    }
    return COREG_OK;
}

static int ref_pivot(coreg_handle* h) {
    HIPCHK(buffer_mean(h, h->ref.p, h->ref_dtype == COREG_F32, (long long)h->gW * h->gH, h->pivots.as<double>(), h->stream));
    return COREG_OK;
}

int coreg_set_reference_on_grid(coreg_handle* h, const void* ref, int dtype, int32_t gy, int32_t gx) {
    if (!h) return COREG_EINVAL;
    if (!ref || gy < 1 || gx < 1 || !is_dtype(dtype))
        return fail(h, COREG_EINVAL, "set_reference_on_grid: bad argument");
    RETCHK(bind_device(h));
    const size_t bytes = (size_t)gy * gx * (dtype == COREG_F32 ? 4 : 8);
    HIPCHK(h->ref.reserve(bytes));
    HIPCHK(hipMemcpyAsync(h->ref.p, ref, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->gW = gx;
    h->gH = gy;
    h->ref_dtype = dtype;
    return ref_pivot(h);
}

// Which pixels of the W x H source image can the once-only resample touch?  The bounding box of the in-bounds sample
// coordinates is computed on the GPU by the same coordinate function the resample uses (k_resample_bbox), widened by the
// spline apron and clipped to the image.  Uploading only that rectangle -- the Carrington grid of the headline touches
// 2 % of the 3072 x 3072 reference, the sub-map of a 2048 x 2048 HRIEUV field 0.6 % -- takes the reference image out of
// the PCIe-inclusive cost of a call; results are bit-identical (same pixels, same arithmetic).  Costs one ~20 us kernel
// and a 4-double read-back.  crop = {0, 0, W, H} when cropping would not pay (more than half the image) or is disabled
// (coreg_set_option "crop_reference" 0).
struct CropRect {
    int x0, y0, w, h;
};
// While the reference smoothing is set (grow_x, grow_y: the reach of its tables) the box is widened by that much before
// it is clipped: every pixel the resample can read is then smoothed from the same taps as in the whole image.
static int reference_crop(coreg_handle* h, int mode, const ResampleArgs& a0, int order, CropRect* out, int grow_x = 0,
                          int grow_y = 0) {
    *out = {0, 0, a0.W, a0.H};
    if (!h->opt_crop_reference || a0.W < 64 || a0.H < 64) return COREG_OK;
    const int nb = 256;
    // On a side stream: the box depends on headers and grid tables only, so it need not queue behind the upload of the
    // image to align that usually precedes it on the handle's stream (its last DMA segment is still in flight).
    if (!h->aux_stream) HIPCHK(hipStreamCreateWithFlags(&h->aux_stream.s, hipStreamNonBlocking));
    HIPCHK(h->bbox_buf.reserve((size_t)nb * 4 * sizeof(double)));
    ResampleArgs a = a0;
    a.bbox = h->bbox_buf.as<double>();
    if (mode == MODE_TRANSLATE)
        hipLaunchKernelGGL((k_resample_bbox<MODE_TRANSLATE>), dim3(nb), dim3(256), 0, h->aux_stream, a);
    else if (mode == MODE_CAR)
        hipLaunchKernelGGL((k_resample_bbox<MODE_CAR>), dim3(nb), dim3(256), 0, h->aux_stream, a);
    else
        hipLaunchKernelGGL((k_resample_bbox<MODE_HOMOGRAPHY>), dim3(nb), dim3(256), 0, h->aux_stream, a);
    HIPCHK(hipGetLastError());
    std::vector<double> part((size_t)nb * 4);
    HIPCHK(hipMemcpyAsync(part.data(), a.bbox, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->aux_stream));
    HIPCHK(hipStreamSynchronize(h->aux_stream));
    double mnx = 1e300, mxx = -1e300, mny = 1e300, mxy = -1e300;
    for (int b = 0; b < nb; ++b) {
        mnx = std::min(mnx, part[4 * b + 0]);
        mxx = std::max(mxx, part[4 * b + 1]);
        mny = std::min(mny, part[4 * b + 2]);
        mxy = std::max(mxy, part[4 * b + 3]);
    }
    const int apron = order / 2 + 3;  // taps of an in-bounds sample: [floor(c) - order/2 - 1, floor(c) + order - order/2 + 1]
    int x0 = 0, x1 = apron * 2, y0 = 0, y1 = apron * 2;  // nothing in bounds: any small rectangle (never read)
    if (mnx <= mxx && mny <= mxy) {
        x0 = std::max(0, (int)std::floor(mnx) - apron);
        x1 = std::min(a0.W - 1, (int)std::floor(mxx) + apron + 1);
        y0 = std::max(0, (int)std::floor(mny) - apron);
        y1 = std::min(a0.H - 1, (int)std::floor(mxy) + apron + 1);
    }
    // (taps that mirror at an image edge stay inside: the rectangle starts AT that edge and is at least 2 aprons wide)
    x1 = std::min(a0.W - 1, std::max(x1, x0 + 2 * apron));
    y1 = std::min(a0.H - 1, std::max(y1, y0 + 2 * apron));
    x0 = std::max(0, x0 - grow_x);
    x1 = std::min(a0.W - 1, x1 + grow_x);
    y0 = std::max(0, y0 - grow_y);
    y1 = std::min(a0.H - 1, y1 + grow_y);
    const long long area = (long long)(x1 - x0 + 1) * (y1 - y0 + 1);
    if (2 * area > (long long)a0.W * a0.H) return COREG_OK;  // not worth a strided copy
    *out = {x0, y0, x1 - x0 + 1, y1 - y0 + 1};
    return COREG_OK;
}

// The reference image's pixels where the resample kernel reads them (*img_dev) and whether they are float32 there.
// Device memory is read where it is, by work enqueued on the handle's stream -- no copy.  From host memory only the
// rectangle the resample can touch crosses PCIe (`crop`, pageable memory only), as the caller or the file stores it:
// float32 pixels (half the PCIe bytes; the reference's float64 cast of them is exact), float64 pixels (tested for
// float32-exactness on the GPU) or the raw big-endian elements of a FITS data unit (decoded on the GPU).
static int upload_reference_source(coreg_handle* h, const void* large, int W, int H, const PixFmt& fmt, bool* f32,
                                   SrcKind kind, const void** img_dev, const CropRect& crop) {
    if (kind == SRC_DEVICE) {
        if (fmt.raw()) return fail(h, COREG_ENOTIMPL, "raw FITS pixels must come from host memory");
        *f32 = fmt.f32;
        *img_dev = large;
        return COREG_OK;
    }
    const size_t n = (size_t)crop.w * crop.h, eb = fmt.elem();
    if (!fmt.raw() && !fmt.f32 && n == (size_t)W * H) {
        // whole float64 image: upload_image stages it itself and, when the pixels are not float32-exact, makes its float64
        // copy the image without another pass
        RETCHK(upload_image(h, (const double*)large, n, h->tmp_img, f32, kind));
        *img_dev = h->tmp_img.p;
        return COREG_OK;
    }
    // which buffer, and how the stored elements get there: float32 pixels (after at most a byte swap) land where the
    // resample reads them, float64 pixels and other FITS elements where their conversion expects them
    DevBuf& dst = fmt.raw() ? (fmt.swap_only() ? h->tmp_img : h->up_raw) : (fmt.f32 ? h->tmp_img : h->up_f64);
    HIPCHK(dst.reserve(n * eb));
    const char* first = (const char*)large + ((size_t)crop.y0 * W + crop.x0) * eb;
    if (kind == SRC_HOST)  // rows of the rectangle packed into pinned staging (whole rows: one contiguous range)
        HIPCHK(stage_to_device(h, RING_CALLER, dst.p, first, (size_t)crop.h, (size_t)crop.w * eb, (size_t)W * eb, h->stream));
    else
        RETCHK(copy_in(h, dst.p, large, n * eb, kind));
    // ... and what makes pixels of them
    *f32 = true;
    if (fmt.raw()) RETCHK(fits_decode(h, fmt, dst.p, n, h->tmp_img, f32));
    else if (!fmt.f32) RETCHK(upload_image(h, h->up_f64.as<double>(), n, h->tmp_img, f32, SRC_DEVICE));
    *img_dev = h->tmp_img.p;
    return COREG_OK;
}

// The half every reference preparation shares, `a` holding the coordinate map of `mode` and the shapes: crop box ->
// source pixels on the device -> once-only resample into h->ref (float32 or float64) -> pivot.
static int prepare_reference(coreg_handle* h, const void* large, const PixFmt& fmt, SrcKind kind, int mode, int order,
                             ResampleArgs& a, bool out_f32) {
    CropRect crop = {0, 0, a.W, a.H};
    const bool smooth = !h->ref_smooth_x.empty();
    // (a pixel's despiked value depends on the source pixels within n_iter x radius of it: the box grows by that much too)
    const int despike_reach = h->has_ref_despike ? h->ref_despike.n_iter * h->ref_despike.radius : 0;
    if (kind == SRC_HOST)
        RETCHK(reference_crop(h, mode, a, order, &crop, despike_reach + (smooth ? (int)h->ref_smooth_x.size() / 2 : 0),
                              despike_reach + (smooth ? (int)h->ref_smooth_y.size() / 2 : 0)));
    const bool carr = mode == MODE_TRANSLATE;
    trace(carr ? "prepare_carrington: crop box known" : "prepare_helioprojective: crop box known");
    bool f32;
    RETCHK(upload_reference_source(h, large, a.W, a.H, fmt, &f32, kind, &a.img, crop));
    h->ref_despike_passes = 0;
    if (h->has_ref_despike) {
        // the pixels the smoothing or the resample reads, despiked into a buffer of the handle (a device source stays as it
        // is); the rim of a rectangle, despiked from a window the rectangle cuts, is never read
        DevBuf* done = nullptr;
        RETCHK(despike_image(h, a.img, f32, crop.h, crop.w, &h->ref_despike, DESPIKE_SLOT_REFERENCE, &done));
        a.img = done->p;
        h->ref_despike_passes = h->ref_despike.n_iter;
    }
    if (smooth) {
        // the pixels the resample reads (the rectangle, or the whole image where it lies: a device source stays as it is)
        // smoothed into a buffer of the handle; the rim of a rectangle, smoothed without its outer taps, is never read
        HIPCHK(h->sm_out.reserve((size_t)crop.w * crop.h * sizeof(double)));
        RETCHK(smooth_image(h, a.img, f32, crop.h, crop.w, h->ref_smooth_y.data(), (long long)h->ref_smooth_y.size(),
                            h->ref_smooth_x.data(), (long long)h->ref_smooth_x.size(), h->sm_out.as<double>()));
        a.img = h->sm_out.p;
        f32 = false;
    }
    if (crop.w != a.W || crop.h != a.H) a.crop = {crop.x0, crop.y0, crop.w};
    HIPCHK(h->ref.reserve((size_t)a.gw * a.gh * (out_f32 ? sizeof(float) : sizeof(double))));
    a.out = h->ref.p;
    RETCHK(dispatch_resample(h, mode, order, f32, out_f32, a, 0));
    h->gW = a.gw;
    h->gH = a.gh;
    h->ref_dtype = out_f32 ? COREG_F32 : COREG_F64;
    RETCHK(ref_pivot(h));
    trace(carr ? "prepare_carrington: issued" : "prepare_helioprojective: issued");
    // no host sync: the pinned staging is guarded by stage_to_device's own wait, everything else is stream-ordered
    return COREG_OK;  // tmp_img stays allocated: the next preparation re-uses it (hipFree would stall the device)
}

static int prepare_carrington(coreg_handle* h, const void* large, const PixFmt& fmt, int32_t ny, int32_t nx,
                              const coreg_wcs2d* hdr, const coreg_carr_grid* grid, double solar_r, int order,
                              SrcKind kind = SRC_HOST) {
    if (!h) return COREG_EINVAL;
    RETCHK(check_image(h, large, ny, nx, "prepare_reference"));
    if (!hdr || !grid) return fail(h, COREG_EINVAL, "prepare_reference: null header or grid");
    RETCHK(check_order(h, order));
    RETCHK(check_wcs(h, hdr, true));
    RETCHK(check_grid(h, grid));
    if (!std::isfinite(solar_r) || !(solar_r > 0.0)) return fail(h, COREG_EINVAL, "solar_r must be positive");
    trace("prepare_carrington: enter");
    RETCHK(bind_device_nowait(h));  // (touches neither the image to align nor its pivot: no join with the upload stream)
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    RETCHK(upload_carr_tables(h, *grid, *hdr, h->has_rot_ref ? &h->rot_ref : nullptr));
    a.carr = carr_dev(h);
    set_carr_common(&a.carr, carr_common(*hdr, solar_r));
    carr_origin(*hdr, &a.x0, &a.y0);
    a.W = nx;
    a.H = ny;
    a.gw = grid->n_lon;
    a.gh = grid->n_lat;
    return prepare_reference(h, large, fmt, kind, MODE_TRANSLATE, order, a, false);
}

static int prepare_helioprojective(coreg_handle* h, const void* large, const PixFmt& fmt, int32_t ny, int32_t nx,
                                   const coreg_wcs2d* hdr_large, const coreg_wcs2d* hdr_small, int order,
                                   SrcKind kind = SRC_HOST) {
    if (!h) return COREG_EINVAL;
    RETCHK(check_image(h, large, ny, nx, "prepare_reference"));
    if (!hdr_large || !hdr_small) return fail(h, COREG_EINVAL, "prepare_reference: null header");
    if (hdr_small->naxis1 < 1 || hdr_small->naxis2 < 1 || too_many(hdr_small->naxis1, hdr_small->naxis2))
        return fail(h, COREG_EINVAL, "hdr_small: NAXIS1/2 missing (or more than 2^31 - 1 pixels)");
    if (hdr_large->proj != hdr_small->proj || (hdr_small->proj != COREG_PROJ_TAN && hdr_small->proj != COREG_PROJ_CAR))
        return fail(h, COREG_ENOTIMPL, "prepare_reference_helioprojective: both headers TAN, or both CAR");
    RETCHK(check_order(h, order));
    RETCHK(check_wcs(h, hdr_large, false));
    RETCHK(check_wcs(h, hdr_small, false));
    RETCHK(bind_device_nowait(h));
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    int mode = MODE_HOMOGRAPHY;
    if (hdr_small->proj == COREG_PROJ_CAR) {
        // two Carrington maps (align_using_initial_carrington: both branches of alignment.py:649-651 / :765-767 build the
        // sub-map for this frame too): pixel of hdr_small -> native angles -> sphere rotation -> native angles of hdr_large
        // -> its pixel, the per-lag map of sweep_car with the roles of the two maps exchanged
        mode = MODE_CAR;
        Mat3 r_small, r_large;
        if (car_native_to_celestial(*hdr_small, &r_small) || car_native_to_celestial(*hdr_large, &r_large))
            return fail(h, COREG_EINVAL, "prepare_reference: no valid native pole for this CRVAL2 / LONPOLE (CAR)");
        const Mat3 m = mat_mul(mat_T(r_large), r_small);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) a.hom.h[3 * i + j] = (double)m.m[i][j];
        set_affine(&a.car_fwd, car_pix_to_native(*hdr_small));
        set_affine(&a.car_inv, car_native_to_pix(*hdr_large));
    } else {
        homography(*hdr_small, *hdr_large, a.hom.h);  // alignment.py:993: pixels of hdr_cut -> pixels of hdr_large
    }
    a.W = nx;
    a.H = ny;
    a.gw = hdr_small->naxis1;
    a.gh = hdr_small->naxis2;
    return prepare_reference(h, large, fmt, kind, mode, order, a, true);
}

// the compressed bytes of a tiled reference image cross PCIe, the pixels never do: decoded into h->dec_img, which the
// preparation then reads as a device source
static int decode_reference_tiled(coreg_handle* h, const coreg_fits_tiled* t, PixFmt* fmt) {
    RETCHK(bind_device(h));
    bool f32;
    RETCHK(decode_tiled_device(h, t, h->dec_img, &f32));
    *fmt = PixFmt::native(f32);
    return COREG_OK;
}

int coreg_prepare_reference_carrington(coreg_handle* h, const double* large, int32_t ny, int32_t nx,
                                       const coreg_wcs2d* hdr, const coreg_carr_grid* grid, double solar_r, int order) {
    return prepare_carrington(h, large, PixFmt::native(false), ny, nx, hdr, grid, solar_r, order);
}

int coreg_prepare_reference_carrington_f32(coreg_handle* h, const float* large, int32_t ny, int32_t nx,
                                           const coreg_wcs2d* hdr, const coreg_carr_grid* grid, double solar_r,
                                           int order) {
    return prepare_carrington(h, large, PixFmt::native(true), ny, nx, hdr, grid, solar_r, order);
}

int coreg_prepare_reference_helioprojective(coreg_handle* h, const double* large, int32_t ny, int32_t nx,
                                            const coreg_wcs2d* hdr_large, const coreg_wcs2d* hdr_small, int order) {
    return prepare_helioprojective(h, large, PixFmt::native(false), ny, nx, hdr_large, hdr_small, order);
}

int coreg_prepare_reference_helioprojective_f32(coreg_handle* h, const float* large, int32_t ny, int32_t nx,
                                                const coreg_wcs2d* hdr_large, const coreg_wcs2d* hdr_small,
                                                int order) {
    return prepare_helioprojective(h, large, PixFmt::native(true), ny, nx, hdr_large, hdr_small, order);
}

int coreg_prepare_reference_carrington_from_device(coreg_handle* h, const void* dev_large, int dtype, int32_t ny,
                                                   int32_t nx, const coreg_wcs2d* hdr_large,
                                                   const coreg_carr_grid* grid, double solar_r, int order) {
    if (h && !is_dtype(dtype)) return fail(h, COREG_EINVAL, "prepare_reference: bad dtype");
    return prepare_carrington(h, dev_large, PixFmt::native(dtype == COREG_F32), ny, nx, hdr_large, grid, solar_r, order,
                              SRC_DEVICE);
}

int coreg_prepare_reference_helioprojective_from_device(coreg_handle* h, const void* dev_large, int dtype, int32_t ny,
                                                        int32_t nx, const coreg_wcs2d* hdr_large,
                                                        const coreg_wcs2d* hdr_small, int order) {
    if (h && !is_dtype(dtype)) return fail(h, COREG_EINVAL, "prepare_reference: bad dtype");
    return prepare_helioprojective(h, dev_large, PixFmt::native(dtype == COREG_F32), ny, nx, hdr_large, hdr_small, order,
                                   SRC_DEVICE);
}

int coreg_prepare_reference_carrington_fits(coreg_handle* h, const coreg_fits_pixels* px, int32_t ny, int32_t nx,
                                            const coreg_wcs2d* hdr_large, const coreg_carr_grid* grid, double solar_r,
                                            int order) {
    if (!h) return COREG_EINVAL;
    PixFmt fmt;
    RETCHK(check_fits(h, px, &fmt));
    return prepare_carrington(h, px->data, fmt, ny, nx, hdr_large, grid, solar_r, order);
}

int coreg_prepare_reference_helioprojective_fits(coreg_handle* h, const coreg_fits_pixels* px, int32_t ny, int32_t nx,
                                                 const coreg_wcs2d* hdr_large, const coreg_wcs2d* hdr_small, int order) {
    if (!h) return COREG_EINVAL;
    PixFmt fmt;
    RETCHK(check_fits(h, px, &fmt));
    return prepare_helioprojective(h, px->data, fmt, ny, nx, hdr_large, hdr_small, order);
}

int coreg_prepare_reference_carrington_tiled(coreg_handle* h, const coreg_fits_tiled* t, const coreg_wcs2d* hdr_large,
                                             const coreg_carr_grid* grid, double solar_r, int order) {
    if (!h) return COREG_EINVAL;
    PixFmt fmt;
    RETCHK(decode_reference_tiled(h, t, &fmt));
    return prepare_carrington(h, h->dec_img.p, fmt, t->naxis2, t->naxis1, hdr_large, grid, solar_r, order, SRC_DEVICE);
}

int coreg_prepare_reference_helioprojective_tiled(coreg_handle* h, const coreg_fits_tiled* t, const coreg_wcs2d* hdr_large,
                                                  const coreg_wcs2d* hdr_small, int order) {
    if (!h) return COREG_EINVAL;
    PixFmt fmt;
    RETCHK(decode_reference_tiled(h, t, &fmt));
    return prepare_helioprojective(h, h->dec_img.p, fmt, t->naxis2, t->naxis1, hdr_large, hdr_small, order, SRC_DEVICE);
}

static int set_rotation(coreg_handle* h, const coreg_diffrot* rot, coreg_diffrot* dst, bool* has) {
    if (!h) return COREG_EINVAL;
    if (rot && !diffrot_valid(*rot)) return fail(h, COREG_EINVAL, "differential rotation: non-finite delta_t or coefficient");
    *has = rot != nullptr;
    if (rot) *dst = *rot;
    return COREG_OK;
}
int coreg_set_reference_rotation(coreg_handle* h, const coreg_diffrot* rot) {
    return h ? set_rotation(h, rot, &h->rot_ref, &h->has_rot_ref) : COREG_EINVAL;
}
int coreg_set_small_rotation(coreg_handle* h, const coreg_diffrot* rot) {
    return h ? set_rotation(h, rot, &h->rot_small, &h->has_rot_small) : COREG_EINVAL;
}

// NaN-aware smoothing of the resident image to align, in place as far as the caller sees: the float64 result is written to
// a buffer of the handle, which then changes places with the image's.
int coreg_smooth_small(coreg_handle* h, const double* wy, int32_t n_wy, const double* wx, int32_t n_wx) {
    if (!h) return COREG_EINVAL;
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    const SmoothPlan p = smooth_plan(h->sH, h->sW, wy, n_wy, wx, n_wx);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);  // (before the join: a refused call changes nothing)
    RETCHK(bind_device(h));                                 // (joins a pending upload: join_small)
    const long long n = (long long)h->sW * h->sH;
    HIPCHK(h->sm_out.reserve((size_t)n * sizeof(double)));
    RETCHK(smooth_image(h, h->small.p, h->small_f32, h->sH, h->sW, wy, n_wy, wx, n_wx, h->sm_out.as<double>()));
    std::swap(h->small, h->sm_out);
    h->small_f32 = false;
    HIPCHK(buffer_mean(h, h->small.p, false, n, h->pivots.as<double>() + 1, h->stream));
    return COREG_OK;
}

int coreg_set_reference_smoothing(coreg_handle* h, const double* wy, int32_t n_wy, const double* wx, int32_t n_wx) {
    if (!h) return COREG_EINVAL;
    if (n_wy == 0 && n_wx == 0) {
        h->ref_smooth_y.clear();
        h->ref_smooth_x.clear();
        return COREG_OK;
    }
    const char* why = smooth_table_refusal(wy, n_wy);
    if (!why) why = smooth_table_refusal(wx, n_wx);
    if (why) return fail(h, COREG_EINVAL, why);
    h->ref_smooth_y.assign(wy, wy + n_wy);
    h->ref_smooth_x.assign(wx, wx + n_wx);
    return COREG_OK;
}

// Median/MAD despiking of the resident image to align, in place as far as the caller sees: the passes write buffers of the
// handle, the last of which then changes places with the image's.  The image keeps the dtype it is held in.
int coreg_despike_small(coreg_handle* h, const coreg_despike_params* params, int64_t* n_flagged) {
    if (!h) return COREG_EINVAL;
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    const DespikePlan p = despike_plan(h->sH, h->sW, params);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);  // (before the join: a refused call changes nothing)
    RETCHK(bind_device(h));                                 // (joins a pending upload: join_small)
    DevBuf* done = nullptr;
    RETCHK(despike_image(h, h->small.p, h->small_f32, h->sH, h->sW, params, DESPIKE_SLOT_IMAGE, &done));
    std::swap(h->small, *done);
    HIPCHK(buffer_mean(h, h->small.p, h->small_f32, (long long)h->sW * h->sH, h->pivots.as<double>() + 1, h->stream));
    if (n_flagged) RETCHK(despike_read_counts(h, DESPIKE_SLOT_IMAGE, params->n_iter, n_flagged));
    return COREG_OK;
}

int coreg_set_reference_despike(coreg_handle* h, const coreg_despike_params* params) {
    if (!h) return COREG_EINVAL;
    if (!params) {
        h->has_ref_despike = false;
        return COREG_OK;
    }
    if (const char* why = despike_params_refusal(params)) return fail(h, COREG_EINVAL, why);
    h->ref_despike = *params;
    h->has_ref_despike = true;
    return COREG_OK;
}

int coreg_last_reference_despike(coreg_handle* h, int64_t* n_flagged8) {
    if (!h) return COREG_EINVAL;
    if (!n_flagged8) return fail(h, COREG_EINVAL, "last_reference_despike: null pointer");
    for (int i = 0; i < kDespikeMaxIter; ++i) n_flagged8[i] = 0;
    if (h->ref_despike_passes < 1) return COREG_OK;  // the last preparation despiked nothing
    RETCHK(bind_device_nowait(h));
    return despike_read_counts(h, DESPIKE_SLOT_REFERENCE, h->ref_despike_passes, n_flagged8);
}

// The planes of a cube despiked one by one and summed over the planes.  It needs no resident image and touches none: the
// work runs in buffers of its own (host_despike_planes.hpp).
int coreg_despike_sum_planes_be(coreg_handle* h, const void* base, int32_t bitpix, int64_t plane_stride, int32_t H, int32_t W,
                                const int64_t* plane_index, int32_t n_sel, const coreg_despike_params* params,
                                double* out_sum, int32_t* out_events, int64_t* n_flagged) {
    if (!h) return COREG_EINVAL;
    return despike_sum_planes(h, base, bitpix, plane_stride, H, W, plane_index, n_sel, params, out_sum, out_events, n_flagged);
}

int coreg_despike_sum_planes_last_ms(coreg_handle* h, double* ms) {
    if (!h || !ms) return COREG_EINVAL;
    if (h->dp_last_ms < 0) return fail(h, COREG_ESTATE, "coreg_despike_sum_planes_be has not run");
    *ms = h->dp_last_ms;
    return COREG_OK;
}

int coreg_get_small(coreg_handle* h, void* out, int dtype) {
    if (!h) return COREG_EINVAL;
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    // float32 pixels may be asked for as float64 (exact); float64 pixels only as they are
    if (!out || !is_dtype(dtype) || (dtype == COREG_F32 && !h->small_f32))
        return fail(h, COREG_EINVAL, "get_small: null pointer, or float32 asked of a float64 image");
    RETCHK(bind_device(h));
    const size_t n = (size_t)h->sW * h->sH;
    if (h->small_f32 && dtype == COREG_F64) {
        std::vector<float> tmp(n);
        HIPCHK(hipMemcpyAsync(tmp.data(), h->small.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (size_t q = 0; q < n; ++q) ((double*)out)[q] = (double)tmp[q];
        return COREG_OK;
    }
    HIPCHK(hipMemcpyAsync(out, h->small.p, n * (h->small_f32 ? sizeof(float) : sizeof(double)), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_get_reference_on_grid(coreg_handle* h, void* out, int dtype) {
    if (!h) return COREG_EINVAL;
    if (!h->ref.p) return fail(h, COREG_ESTATE, "no reference image on the target grid");
    if (!out || dtype != h->ref_dtype) return fail(h, COREG_EINVAL, "get_reference_on_grid: dtype mismatch");
    RETCHK(bind_device(h));
    const size_t bytes = (size_t)h->gW * h->gH * (dtype == COREG_F32 ? 4 : 8);
    HIPCHK(hipMemcpyAsync(out, h->ref.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_resample_carrington(coreg_handle* h, const coreg_wcs2d* hdr, const coreg_carr_grid* grid, double solar_r,
                              int order, double* out) {
    if (!h) return COREG_EINVAL;
    if (!hdr || !grid || !out) return fail(h, COREG_EINVAL, "resample_carrington: bad argument");
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    RETCHK(check_order(h, order));
    RETCHK(check_wcs(h, hdr, true));
    RETCHK(check_grid(h, grid));
    if (!std::isfinite(solar_r) || !(solar_r > 0.0)) return fail(h, COREG_EINVAL, "solar_r must be positive");
    RETCHK(bind_device(h));
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    RETCHK(upload_carr_tables(h, *grid, *hdr, h->has_rot_small ? &h->rot_small : nullptr));
    a.carr = carr_dev(h);
    set_carr_common(&a.carr, carr_common(*hdr, solar_r));
    carr_origin(*hdr, &a.x0, &a.y0);
    a.img = h->small.p;
    a.W = h->sW;
    a.H = h->sH;
    a.gw = grid->n_lon;
    a.gh = grid->n_lat;
    const size_t bytes = (size_t)a.gw * a.gh * sizeof(double);
    HIPCHK(h->out_dev.reserve(bytes));
    a.out = h->out_dev.p;
    RETCHK(dispatch_resample(h, MODE_TRANSLATE, order, h->small_f32, false, a, 0));
    HIPCHK(hipMemcpyAsync(out, h->out_dev.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

static int resample_helio(coreg_handle* h, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr, int order, void* out,
                          bool out_f32) {
    if (!h) return COREG_EINVAL;
    if (!hdr_target || !hdr || !out) return fail(h, COREG_EINVAL, "resample_helioprojective: bad argument");
    if (!h->small.p) return fail(h, COREG_ESTATE, "coreg_set_small has not been called");
    if (hdr_target->naxis1 < 1 || hdr_target->naxis2 < 1 || too_many(hdr_target->naxis1, hdr_target->naxis2))
        return fail(h, COREG_EINVAL, "hdr_target: NAXIS missing (or more than 2^31 - 1 pixels)");
    RETCHK(check_order(h, order));
    RETCHK(check_wcs(h, hdr_target, false));
    RETCHK(check_wcs(h, hdr, false));
    RETCHK(bind_device(h));
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    if (hdr_target->proj != COREG_PROJ_TAN || hdr->proj != COREG_PROJ_TAN)
        return fail(h, COREG_ENOTIMPL, "resample_helioprojective: TAN headers only");
    homography(*hdr_target, *hdr, a.hom.h);  // alignment.py:1022
    a.img = h->small.p;
    a.W = h->sW;
    a.H = h->sH;
    a.gw = hdr_target->naxis1;
    a.gh = hdr_target->naxis2;
    const size_t bytes = (size_t)a.gw * a.gh * (out_f32 ? sizeof(float) : sizeof(double));
    HIPCHK(h->out_dev.reserve(bytes));
    a.out = h->out_dev.p;
    RETCHK(dispatch_resample(h, MODE_HOMOGRAPHY, order, h->small_f32, out_f32, a, 0));
    HIPCHK(hipMemcpyAsync(out, h->out_dev.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

int coreg_resample_helioprojective(coreg_handle* h, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr, int order,
                                   float* out) {
    return resample_helio(h, hdr_target, hdr, order, out, true);
}

int coreg_resample_helioprojective_f64(coreg_handle* h, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr,
                                       int order, double* out) {
    return resample_helio(h, hdr_target, hdr, order, out, false);
}
}  // extern "C"
