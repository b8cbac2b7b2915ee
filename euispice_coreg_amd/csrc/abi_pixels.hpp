// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the C ABI of the integer
// pixel-lag sweep (include/coreg_hip.h).
#pragma once

extern "C" {

int coreg_pixels_set_large(coreg_handle* h, const void* img, int dtype, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    return pixels_set_large(h, img, dtype, ny, nx);
}

int coreg_pixels_set_small(coreg_handle* h, const void* img, int dtype, int32_t ny, int32_t nx) {
    if (!h) return COREG_EINVAL;
    return pixels_set_small(h, img, dtype, ny, nx);
}

int coreg_pixels_shift_large(coreg_handle* h, double dx, double dy) {
    if (!h) return COREG_EINVAL;
    return pixels_shift_large(h, dx, dy);
}

int coreg_pixels_smooth_large(coreg_handle* h, const double* wy, int32_t n_wy, const double* wx, int32_t n_wx) {
    if (!h) return COREG_EINVAL;
    return pixels_smooth(h, 0, wy, n_wy, wx, n_wx);
}

int coreg_pixels_smooth_small(coreg_handle* h, const double* wy, int32_t n_wy, const double* wx, int32_t n_wx) {
    if (!h) return COREG_EINVAL;
    return pixels_smooth(h, 1, wy, n_wy, wx, n_wx);
}

int coreg_pixels_despike_large(coreg_handle* h, const coreg_despike_params* params, int64_t* n_flagged) {
    if (!h) return COREG_EINVAL;
    return pixels_despike(h, 0, params, n_flagged);
}

int coreg_pixels_despike_small(coreg_handle* h, const coreg_despike_params* params, int64_t* n_flagged) {
    if (!h) return COREG_EINVAL;
    return pixels_despike(h, 1, params, n_flagged);
}

int coreg_pixels_get_image(coreg_handle* h, int which, double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_get_image(h, which, out);
}

int coreg_pixels_sweep_method(coreg_handle* h, const coreg_pixels_plan* plan, int method, double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_sweep(h, plan, method, out);
}

int coreg_pixels_sweep(coreg_handle* h, const coreg_pixels_plan* plan, double* corr_out) {
    return coreg_pixels_sweep_method(h, plan, COREG_METHOD_CORRELATION, corr_out);
}

int coreg_pixels_set_bins(coreg_handle* h, const double* edges_small, int32_t n_small, const double* edges_large,
                          int32_t n_large) {
    if (!h) return COREG_EINVAL;
    return pixels_set_bins(h, edges_small, n_small, edges_large, n_large);
}

int coreg_pixels_last_counts(coreg_handle* h, double* dst) {
    if (!h) return COREG_EINVAL;
    return pixels_last_counts(h, dst);
}

int coreg_pixels_sweep_tiles(coreg_handle* h, const coreg_pixels_plan* plan, int method, int32_t tile_ny, int32_t tile_nx,
                             double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_sweep_tiles(h, plan, method, tile_ny, tile_nx, out);
}

int coreg_pixels_last_tile_counts(coreg_handle* h, double* dst) {
    if (!h) return COREG_EINVAL;
    return pixels_last_tile_counts(h, dst);
}

int coreg_pixels_sweep_windows(coreg_handle* h, const coreg_pixels_plan* plan, int method, int32_t tile_ny, int32_t tile_nx,
                               int32_t step_ny, int32_t step_nx, const double* wy, const double* wx, double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_sweep_windows(h, plan, method, tile_ny, tile_nx, step_ny, step_nx, wy, wx, out);
}

int coreg_pixels_last_tile_weights(coreg_handle* h, double* dst) {
    if (!h) return COREG_EINVAL;
    return pixels_last_tile_weights(h, dst);
}

int coreg_pixels_get_large_box(coreg_handle* h, double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_get_large_box(h, out);
}

int coreg_pixels_get_rotated(coreg_handle* h, int32_t k, double* out) {
    if (!h) return COREG_EINVAL;
    return pixels_get_rotated(h, k, out);
}

int coreg_pixels_last_timing(coreg_handle* h, double* ms) {
    if (!h) return COREG_EINVAL;
    return pixels_last_timing(h, ms);
}

int coreg_pixels_destretch(coreg_handle* h, const void* cube, int dtype, int32_t n_planes, int32_t ny, int32_t nx,
                           const coreg_pixels_field* f, void* out, double* displacement) {
    if (!h) return COREG_EINVAL;
    return pixels_destretch(h, cube, dtype, n_planes, ny, nx, f, out, displacement);
}

int coreg_pixels_destretch_last_ms(coreg_handle* h, double* ms) {
    if (!h) return COREG_EINVAL;
    return pixels_destretch_last_ms(h, ms);
}

}  // extern "C"
