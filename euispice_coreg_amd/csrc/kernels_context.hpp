// Part of csrc/kernels.hpp (included from there in order): the iterative-context sweep of
// AlignementSpiceIterativeContextRaster (hdrshift/alignment_spice.py:357-469 of the reference).  For every lag-point the
// reference composes a synthetic raster on the SHIFTED SPICE grid (each column an order-2 sample of the imager frame
// nearest in time to that slit, synras/map_builder.py:89-131), resamples the SPICE image onto the same grid
// (alignment.py:1018-1029, float32 destination) and correlates the two (c_correlate.py:39-72) or takes `residus`.
// Here both samples of every (grid point, lag) are taken in ONE kernel:
//   a = order-2 sample of frame col_frame[i] at H_ctx(frame, lag) (i, j)   (float32-rounded when the frames are float32)
//   b = order-N sample of the SPICE image at H_sp(lag) (i, j)              (always float32-rounded)
// and the six Pearson sums go out in the layout of k_sweep's partial slabs ([group][kNumSums][n_slots]), so that
// k_finalize / k_refine_list finish them unchanged.  Work: one workgroup per (group of kCtxCols raster columns,
// kCtxLags lag slots); a column takes one frame, so a workgroup reads one or two frames, along a line of them that the
// L2 keeps (no LDS staging: the taps of neighbouring rows overlap in cache, and a frame of 2048^2 does not fit an LDS).
// Samples are exact per point (no incremental map); the deterministic LDS tree adds a workgroup's 256 lanes.
#pragma once
namespace coreg {

constexpr int kCtxThreads = 256;
constexpr int kCtxCols = 2;  // raster columns per point group
constexpr int kCtxLags = 8;  // lag slots per workgroup

struct ContextArgs {
    const void* frames;  // [n_frames][fH][fW] float / double
    int frames_f32;
    int fW, fH;
    const int* col_frame;  // [gW] frame of every raster column
    int n_frames;
    const void* small;  // SPICE image [sH][sW]
    int small_f32;
    int sW, sH, order;
    int gW, gH;            // target grid (the shifted SPICE grid)
    const double* h_ctx;   // [n_slots][n_frames][9] grid pixel -> frame pixel
    const double* h_sp;    // [n_slots][9] grid pixel -> SPICE pixel of the shifted header (near identity)
    // noise-decided bounds rule of the SPICE sample on the grid's border pixels (wcslib's own arithmetic, host):
    // [n_slots][2 (gH + gW)] (left column, right column, top row, bottom row): 0 the map decides, 1 inside, 2 outside
    const unsigned char* edge;
    int has_min, has_max;
    float vmin, vmax;  // thresholds on the float32 SPICE sample (compared in float32, alignment_spice.py:396-399)
    int residus;  // 0: Pearson, 1: 'residus', 2: 'residus_masked'
    long long n_slots;
    double pa, pb;      // pivots of the sums (context, SPICE)
    double* partials;   // [n_groups][kNumSums][n_slots]
};

template <typename TF, typename TS>
__device__ __forceinline__ void ctx_pair(const ContextArgs& c, long long slot, int i, int j, double& a, double& b) {
    const double nan = __builtin_nan("");
    const double x = (double)i, y = (double)j;
    const int f = c.col_frame[i];
    const double* hc = c.h_ctx + ((size_t)slot * c.n_frames + f) * 9;
    double w = fma(hc[6], x, fma(hc[7], y, hc[8]));
    const double fx = fma(hc[0], x, fma(hc[1], y, hc[2])) / w;
    const double fy = fma(hc[3], x, fma(hc[4], y, hc[5])) / w;
    bool inb;
    const TF* fr = (const TF*)c.frames + (size_t)f * c.fW * c.fH;
    const double av = spline_global_rt<TF>(fr, c.fW, c.fH, fx, fy, 2, inb);
    a = inb ? (c.frames_f32 ? (double)(float)av : av) : nan;  // interpol2d into an array of the frame's dtype

    const double* hs = c.h_sp + (size_t)slot * 9;
    w = fma(hs[6], x, fma(hs[7], y, hs[8]));
    double sx = fma(hs[0], x, fma(hs[1], y, hs[2])) / w;
    double sy = fma(hs[3], x, fma(hs[4], y, hs[5])) / w;
    int e = 0;
    if (c.edge && (i == 0 || i == c.gW - 1 || j == 0 || j == c.gH - 1)) {
        const unsigned char* ed = c.edge + (size_t)slot * (2 * (c.gW + c.gH));
        if (i == 0) e |= ed[j];
        if (i == c.gW - 1) e |= ed[c.gH + j];
        if (j == 0) e |= ed[2 * c.gH + i];
        if (j == c.gH - 1) e |= ed[2 * c.gH + c.gW + i];
    }
    if (e & 2) {
        b = nan;
        return;
    }
    if (e & 1) {  // wcslib puts it inside: a coordinate the exact map left ~1e-12 px outside is taken on the bound
        sx = fmin(fmax(sx, 0.0), (double)(c.sW - 1));
        sy = fmin(fmax(sy, 0.0), (double)(c.sH - 1));
    }
    const double bv = spline_global_rt<TS>((const TS*)c.small, c.sW, c.sH, sx, sy, c.order, inb);
    b = inb ? (double)(float)bv : nan;  // float32 destination (alignment.py:1024)
}

__device__ __forceinline__ bool ctx_selected(const ContextArgs& c, double b) {
    const float bf = (float)b;  // (b is float32-exact or NaN; NaN fails both comparisons)
    return (!c.has_min || bf > c.vmin) && (!c.has_max || bf < c.vmax);
}

// Adds one (a, b) pair to the six sums: Pearson moments about (pa, pb) with the NaN mask, or, for 'residus',
// d = (a - b) / sqrt(a) in slots 2 and 4 over the thresholded points only, NaN included (no NaN mask in the reference's
// _step: one NaN makes the lag-point NaN, alignment_spice.py:416-419)
__device__ __forceinline__ void ctx_accumulate(const ContextArgs& c, double a, double b, double pa, double pb,
                                               double s[kNumSums]) {
    if (!ctx_selected(c, b) && (c.has_min || c.has_max)) return;
    if (c.residus == 2) {  // 'residus_masked': co-finite samples only; a term that is not finite poisons (sum 1)
        if (!isfinite(a) || !isfinite(b)) return;
        const double d = (a - b) / sqrt(a);
        if (isfinite(d)) {
            s[0] += 1.0;
            s[2] += d;
            s[4] += d * d;
        } else {
            s[1] += 1.0;
        }
        return;
    }
    if (c.residus) {
        const double d = (a - b) / sqrt(a);
        s[0] += 1.0;
        s[2] += d;
        s[4] += d * d;
        return;
    }
    if (a != a || b != b) return;
    const double da = a - pa, db = b - pb;
    s[0] += 1.0;
    s[1] += da;
    s[2] += db;
    s[3] += da * da;
    s[4] += db * db;
    s[5] += da * db;
}

// fixed-order tree over the workgroup's lanes; the result is in red[k][0]
__device__ __forceinline__ void ctx_block_sum(double (*red)[kCtxThreads], const double s[kNumSums]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kNumSums; ++k) red[k][t] = s[k];
    __syncthreads();
    for (int w = kCtxThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < kNumSums; ++k) red[k][t] += red[k][t + w];
        }
        __syncthreads();
    }
}

template <typename TF, typename TS>
__global__ void __launch_bounds__(kCtxThreads) k_context_sweep(const ContextArgs c) {
    __shared__ double red[kNumSums][kCtxThreads];
    const int g = blockIdx.x;
    const int c0 = g * kCtxCols;
    const int ncols = min(kCtxCols, c.gW - c0);
    const int npts = ncols * c.gH;
    const long long slot0 = (long long)blockIdx.y * kCtxLags;
    for (int q = 0; q < kCtxLags; ++q) {
        const long long slot = slot0 + q;
        if (slot >= c.n_slots) break;  // (uniform)
        double s[kNumSums];
#pragma unroll
        for (int k = 0; k < kNumSums; ++k) s[k] = 0.0;
        for (int p = threadIdx.x; p < npts; p += kCtxThreads) {
            const int i = c0 + p / c.gH, j = p % c.gH;  // down a column: one frame, neighbouring rows
            double a, b;
            ctx_pair<TF, TS>(c, slot, i, j, a, b);
            ctx_accumulate(c, a, b, c.pa, c.pb, s);
        }
        ctx_block_sum(red, s);
        if (threadIdx.x < kNumSums)
            c.partials[((size_t)g * kNumSums + threadIdx.x) * c.n_slots + slot] = red[threadIdx.x][0];
        __syncthreads();
    }
}

// 'residus': np.std over the thresholded samples (one-pass moments, as k_finalize's residus branch); NaN when a selected
// sample is NaN or nothing is selected, and when a term is infinite (a = 0 with b != 0): np.std's mean is then infinite,
// its deviations NaN, while s4 / n - m * m would be inf - inf and fmax(NaN, 0) = 0, the best possible score.  (Unlike the
// main sweeps, whose point_lag drops a non-finite term, ctx_accumulate adds every selected term.)
// 'residus_masked' (masked = 1): the terms are finite by construction; NaN when nothing is co-finite and selected, or
// when a poisoned term was met (sum 1, ctx_accumulate).  `counts` (or null): n per lag-point, as FinalizeArgs.counts.
__global__ void k_finalize_context_residus(const double* partials, int n_groups, long long n_slots,
                                           long long lag_begin, const long long* out_index, double* out, int masked,
                                           double* counts) {
    const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    double n = 0.0, s1 = 0.0, s2 = 0.0, s4 = 0.0;
    for (int g = 0; g < n_groups; ++g) {
        const double* p = partials + (size_t)g * kNumSums * n_slots + slot;
        n += p[0];
        s1 += p[n_slots];
        s2 += p[2 * n_slots];
        s4 += p[4 * n_slots];
    }
    double r = __builtin_nan("");
    if (n > 0.0 && isfinite(s2) && s4 == s4 && (!masked || s1 == 0.0)) {
        // m * m rounded on its own, not fused with the subtraction: the fma would leave the product's rounding error
        // (up to half an ulp of m * m), so one selected sample, or equal terms, would give sqrt(that) instead of 0
#pragma clang fp contract(off)
        const double m = s2 / n;
        r = sqrt(fmax(s4 / n - m * m, 0.0));
    }
    out[out_index[slot] - lag_begin] = r;
    if (counts) counts[out_index[slot] - lag_begin] = n;
}

// Re-evaluation of the lag-points k_finalize flagged (list from k_refine_list): one workgroup per flagged slot walks the
// whole grid again with the slot's own means as pivots and writes the corrected two-pass coefficient (as k_refine).
template <typename TF, typename TS>
__global__ void __launch_bounds__(kCtxThreads) k_refine_context(const ContextArgs c, const RefineArgs r) {
    __shared__ double red[kNumSums][kCtxThreads];
    const int n = r.head[0];
    const long long npts = (long long)c.gW * c.gH;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const int slot = r.list[e];
        const double pa = c.pa + r.slot_pivots[slot], pb = c.pb + r.slot_pivots[c.n_slots + slot];
        double s[kNumSums];
#pragma unroll
        for (int k = 0; k < kNumSums; ++k) s[k] = 0.0;
        for (long long p = threadIdx.x; p < npts; p += kCtxThreads) {
            const int i = (int)(p / c.gH), j = (int)(p % c.gH);
            double a, b;
            ctx_pair<TF, TS>(c, slot, i, j, a, b);
            ctx_accumulate(c, a, b, pa, pb, s);
        }
        ctx_block_sum(red, s);
        if (threadIdx.x == 0) {
            const double cnt = red[0][0];
            double res = __builtin_nan("");
            if (cnt > 1.0) {
                const double cov = red[5][0] - red[1][0] * red[2][0] / cnt;
                const double va = red[3][0] - red[1][0] * red[1][0] / cnt;
                const double vb = red[4][0] - red[2][0] * red[2][0] / cnt;
                res = cov / sqrt(va * vb);
            }
            r.out[r.out_index[slot] - r.lag_begin] = res;
            if (r.counts) r.counts[r.out_index[slot] - r.lag_begin] = cnt;
        }
        __syncthreads();
    }
}

// one frame of the stack from the decoded image-to-align buffer (raw FITS / Rice frames go through the upload paths of
// coreg_set_small_fits / _tiled, then here)
template <typename TD, typename TSRC>
__global__ void k_ctx_copy_frame(TD* dst, const TSRC* src, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = (TD)src[i];
}

}  // namespace coreg
