// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the C ABI of the
// iterative-context sweep (include/coreg_hip.h).
#pragma once

extern "C" {

int coreg_set_context_frames(coreg_handle* h, int32_t n_frames, int32_t ny, int32_t nx, int dtype,
                             const coreg_wcs2d* hdrs, const void* const* pixels) {
    if (!h) return COREG_EINVAL;
    return context_set_frames(h, n_frames, ny, nx, dtype, hdrs, pixels);
}

int coreg_context_frame_from_small(coreg_handle* h, int32_t k) {
    if (!h) return COREG_EINVAL;
    return context_frame_from_small(h, k);
}

int coreg_sweep_context(coreg_handle* h, const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr_small,
                        const int32_t* col_frame, const coreg_lags* lags, int order, int method, int cdelt_semantics,
                        int has_min, double vmin, int has_max, double vmax, int64_t lag_begin, int64_t lag_end,
                        double* corr_out, int out_on_device) {
    if (!h) return COREG_EINVAL;
    return context_sweep(h, hdr_target, hdr_small, col_frame, lags, order, method, cdelt_semantics, has_min, vmin,
                         has_max, vmax, lag_begin, lag_end, corr_out, out_on_device);
}

int coreg_context_lag_headers(const coreg_wcs2d* hdr_target, const coreg_wcs2d* hdr_small, double d_crval1,
                              double d_crval2, double d_cdelt1, double d_cdelt2, double d_crota, int cdelt_semantics,
                              coreg_wcs2d* ctx, coreg_wcs2d* grid, coreg_wcs2d* shifted) {
    if (!hdr_target || !hdr_small || !ctx || !grid || !shifted) return COREG_EINVAL;
    return context_lag_headers(*hdr_target, *hdr_small, d_crval1, d_crval2, d_cdelt1, d_cdelt2, d_crota,
                               cdelt_semantics, ctx, grid, shifted);
}

}  // extern "C"
