// Median/MAD despiking of an image (the rule, the geometry and the decision: despike_plan.hpp).
//   k_despike<T, R>  one pass (Jacobi: every decision is taken on `src`, every pixel of `dst` is written).  A work item is a
//                    tile of 32 x 8 pixels; the tile and its R-wide halo stand in LDS as float64, NaN for a pixel that is
//                    not finite or lies outside the image, so that the clipped window needs no branch.  Thread t reads the
//                    (2R+1)^2 - 1 neighbours of its pixel into registers (R is a template parameter: the loops unroll, no
//                    index is a run-time one) and calls despike_decide, which the host walks too.  The two selections are
//                    sorting networks: comparisons only, no data-dependent branch, the same instructions for every lane.
//                    The flagged pixels of a workgroup are counted by ballot and added to *n_flagged with ONE integer
//                    atomicAdd; there is no floating-point atomic.
// Workgroups loop over the work items (grid-stride), so no image size meets a grid limit; pixel offsets are 64-bit.
#pragma once
#include "despike_plan.hpp"

namespace coreg {

template <typename T, int R>
__global__ __launch_bounds__(kDespikeThreads) void k_despike(const T* __restrict__ src, T* __restrict__ dst, DespikeGeom g,
                                                              coreg_despike_params prm,
                                                              unsigned long long* __restrict__ n_flagged) {
    constexpr int NN = despike_neighbours(R);
    constexpr int pitch = despike_lds_pitch(R);
    __shared__ double win[despike_lds_entries(R)];
    __shared__ unsigned wave_count[kDespikeThreads / 64];
    const int t = (int)threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    unsigned mine = 0;  // flagged pixels of this thread's wave (the same in all its lanes)
    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        int y0, x0;
        despike_origin(g, item, &y0, &x0);
        for (int e = t; e < despike_lds_entries(R); e += kDespikeThreads) {
            const long long y = (long long)y0 - R + e / pitch, x = (long long)x0 - R + e % pitch;
            double v = nan;
            if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
                const double p = (double)src[y * g.W + x];
                if (isfinite(p)) v = p;
            }
            win[e] = v;
        }
        __syncthreads();
        int row, col;
        bool flagged = false;
        if (despike_pixel(g, item, t, &row, &col)) {
            const long long q = (long long)row * g.W + col;
            const T stored = src[q];
            T result = stored;
            if (isfinite(stored)) {
                double n[NN];
                int s = 0;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx)
                        if (dy != 0 || dx != 0) n[s++] = win[despike_lds_index(R, t, dy, dx)];
                const DespikeDecision dec = despike_decide<NN>((double)stored, n, prm);
                flagged = dec.flagged;
                if (flagged) result = prm.replace == COREG_DESPIKE_MEDIAN ? (T)dec.med : (T)nan;
            }
            dst[q] = result;
        }
        mine += (unsigned)__popcll(__ballot(flagged));
        __syncthreads();
    }
    if ((t & 63) == 0) wave_count[t >> 6] = mine;
    __syncthreads();
    if (t == 0) {
        unsigned total = 0;
        for (int w = 0; w < kDespikeThreads / 64; ++w) total += wave_count[w];
        if (total) atomicAdd(n_flagged, (unsigned long long)total);
    }
}

}  // namespace coreg
