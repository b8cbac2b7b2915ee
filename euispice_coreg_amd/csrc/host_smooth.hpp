// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the NaN-aware separable
// smoothing of a resident image -- the plan (csrc/smooth_plan.hpp: table checks, geometry; no GPU work)
// and the two launches (csrc/kernels_smooth.hpp) on the handle's stream.
#pragma once
namespace {

// H x W pixels at `src` (float32 or float64, rows packed) smoothed into the float64 image `out`; `out` may be `src` when
// that is float64.  The planes num and den are work space of the handle.  Every check comes before any GPU work.
int smooth_image(coreg_handle* h, const void* src, bool f32, int H, int W, const double* wy, long long n_wy,
                 const double* wx, long long n_wx, double* out) {
    const SmoothPlan p = smooth_plan(H, W, wy, n_wy, wx, n_wx);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);
    SmoothTable ty, tx;
    smooth_table_fill(&ty, wy, (int)n_wy);
    smooth_table_fill(&tx, wx, (int)n_wx);
    const size_t bytes = (size_t)H * W * sizeof(double);
    HIPCHK(h->sm_num.reserve(bytes));
    HIPCHK(h->sm_den.reserve(bytes));
    double* num = h->sm_num.as<double>();
    double* den = h->sm_den.as<double>();
    const dim3 block(kSmoothThreads);
    if (f32) {
        hipLaunchKernelGGL((k_smooth_rows<float>), dim3(p.row_grid), block, 0, h->stream, (const float*)src, p.g, tx, num, den);
        hipLaunchKernelGGL((k_smooth_cols<float>), dim3(p.col_grid), block, p.col_lds, h->stream, (const float*)src, p.g, ty,
                           num, den, out);
    } else {
        hipLaunchKernelGGL((k_smooth_rows<double>), dim3(p.row_grid), block, 0, h->stream, (const double*)src, p.g, tx, num,
                           den);
        hipLaunchKernelGGL((k_smooth_cols<double>), dim3(p.col_grid), block, p.col_lds, h->stream, (const double*)src, p.g, ty,
                           num, den, out);
    }
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

}  // namespace
