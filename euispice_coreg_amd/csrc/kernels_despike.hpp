// Median/MAD despiking (the rule, the tiles and the decision: despike_plan.hpp; the
// stack of planes and its sum: despike_planes_plan.hpp).  The pixels stand on the device as a packed stack [n][H][W] of
// float32 or float64, as a FITS file stores them (`be`: big-endian, the byte swap is the load) or in native order; a
// resident image is one plane in native order.
// The contract of the kernels, stated once: a work item is a tile of 32 x 8
// pixels of one plane, one pixel per thread.  The tile and its R-wide halo stand in LDS as float64, NaN for a pixel that
// is not finite or lies outside the plane, so that the clipped window needs no branch and never reaches into another
// plane.  Thread t reads the (2R+1)^2 - 1 neighbours of its pixel into registers (R is a template parameter: the loops
// unroll, no index is a run-time one) and calls despike_decide, which the host walks too.  The two selections are sorting
// networks: comparisons only, no data-dependent branch, the same instructions for every lane.  A pixel that is not finite
// is never a neighbour and never changes; a flagged pixel becomes NaN or the median rounded to T.  Every decision of a pass
// is taken on its input (Jacobi).  The flag events of a workgroup are counted by ballot and added to *n_flagged with ONE
// integer atomicAdd; there is no floating-point atomic.  Workgroups loop over their work items (grid-stride), so no size
// meets a grid limit; pixel offsets are 64-bit.
//   k_despike_image<T, R>        one pass of a resident image: writes every pixel of `dst`.  It stages its window with
//                                despike_window_entry like the other two, but carries its own copy of the gather,
//                                decide and replace block (despike_replace) and of the count tail (despike_add_count):
//                                every form of it built on those two, and the image run through k_despike_planes_pass
//                                as a stack of one plane, compiled to other code for the sorting networks and measured
//                                up to 5 % slower.  As it stands its code is, instruction for
//                                instruction, what it was before the planes' kernels came.  A change to the rule goes
//                                into both copies; tests/test_gpu_despike_planes.py holds them to each other.
//   k_despike_planes_pass<T, R>  a pass of a stack of planes that is not the last (n_iter > 1), over (plane, tile) pairs:
//                                writes every pixel of the despiked stack and adds a flag event to the int32 map (one entry
//                                per pixel of a plane) by integer atomicAdd.
//   k_despike_planes_sum<T, R>   the last pass of a stack of planes, fused with the sum.  A workgroup owns a tile and walks
//                                the planes in order: thread t decides its pixel and adds the despiked value to its running
//                                float64 sum (despike_planes_add: the order of the additions is the order of the loop); the
//                                events of its pixel are counted in a register.  It writes `sum` and `events` alone: no
//                                despiked stack.  With `overlap` the window of plane k + 1 is loaded into registers before
//                                plane k's sorting networks and written to the second LDS window after them, so that a
//                                workgroup meets the latency of global memory once per tile, not once per plane; one barrier
//                                per plane either way.
#pragma once
#include "despike_planes_plan.hpp"

namespace coreg {

// element i of a stack as the file stores it (`be`: big-endian) or in native order
__device__ __forceinline__ float despike_load(const float* p, long long i, bool be) {
    const unsigned u = ((const unsigned*)p)[i];
    return __uint_as_float(be ? __builtin_bswap32(u) : u);
}
__device__ __forceinline__ double despike_load(const double* p, long long i, bool be) {
    const unsigned long long u = ((const unsigned long long*)p)[i];
    return __longlong_as_double((long long)(be ? __builtin_bswap64(u) : u));
}

// what entry e of the staged window of the tile at (y0, x0) holds: the pixel as float64, NaN where it is not finite, lies
// outside the plane, or e is past the window
template <typename T, int R>
__device__ __forceinline__ double despike_window_entry(const T* __restrict__ plane, bool be, const DespikeGeom& g, int y0,
                                                       int x0, int e) {
    constexpr int pitch = despike_lds_pitch(R);
    const long long y = (long long)y0 - R + e / pitch, x = (long long)x0 - R + e % pitch;
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (e < despike_lds_entries(R) && y >= 0 && y < g.H && x >= 0 && x < g.W) {
        const double p = (double)despike_load(plane, y * g.W + x, be);
        if (isfinite(p)) v = p;
    }
    return v;
}

// thread t's pixel `stored` against the staged window: true when flagged; *result is the despiked pixel
template <typename T, int R>
__device__ __forceinline__ bool despike_replace(const double* win, int t, T stored, const coreg_despike_params& prm, T* result) {
    constexpr int NN = despike_neighbours(R);
    *result = stored;
    if (!isfinite(stored)) return false;
    double n[NN];
    int s = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx)
            if (dy != 0 || dx != 0) n[s++] = win[despike_lds_index(R, t, dy, dx)];
    const DespikeDecision dec = despike_decide<NN>((double)stored, n, prm);
    if (dec.flagged) *result = prm.replace == COREG_DESPIKE_MEDIAN ? (T)dec.med : (T)__longlong_as_double(0x7ff8000000000000ll);
    return dec.flagged;
}

// the flag events of a workgroup (`mine`: those of the thread's wave, the same in all its lanes) added to *n_flagged
__device__ __forceinline__ void despike_add_count(unsigned mine, unsigned* wave_count, unsigned long long* n_flagged) {
    const int t = (int)threadIdx.x;
    if ((t & 63) == 0) wave_count[t >> 6] = mine;
    __syncthreads();
    if (t == 0) {
        unsigned total = 0;
        for (int w = 0; w < kDespikeThreads / 64; ++w) total += wave_count[w];
        if (total) atomicAdd(n_flagged, (unsigned long long)total);
    }
}

template <typename T, int R>
__global__ __launch_bounds__(kDespikeThreads) void k_despike_image(const T* __restrict__ src, T* __restrict__ dst, DespikeGeom g,
                                                                    coreg_despike_params prm,
                                                                    unsigned long long* __restrict__ n_flagged) {
    constexpr int NN = despike_neighbours(R);
    __shared__ double win[despike_lds_entries(R)];
    __shared__ unsigned wave_count[kDespikeThreads / 64];
    const int t = (int)threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    unsigned mine = 0;  // flagged pixels of this thread's wave (the same in all its lanes)
    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        int y0, x0;
        despike_origin(g, item, &y0, &x0);
        for (int e = t; e < despike_lds_entries(R); e += kDespikeThreads) win[e] = despike_window_entry<T, R>(src, false, g, y0, x0, e);
        __syncthreads();
        int row, col;
        bool flagged = false;
        if (despike_pixel(g, item, t, &row, &col)) {
            const long long q = (long long)row * g.W + col;
            const T stored = src[q];
            T result = stored;
            if (isfinite(stored)) {  // (this kernel's copy of despike_replace)
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
    if ((t & 63) == 0) wave_count[t >> 6] = mine;  // (this kernel's copy of despike_add_count)
    __syncthreads();
    if (t == 0) {
        unsigned total = 0;
        for (int w = 0; w < kDespikeThreads / 64; ++w) total += wave_count[w];
        if (total) atomicAdd(n_flagged, (unsigned long long)total);
    }
}

template <typename T, int R>
__global__ __launch_bounds__(kDespikeThreads) void k_despike_planes_pass(const T* __restrict__ src, bool be, T* __restrict__ dst,
                                                                          DespikeGeom g, long long plane_px, long long pairs,
                                                                          coreg_despike_params prm, int* __restrict__ events,
                                                                          unsigned long long* __restrict__ n_flagged) {
    __shared__ double win[despike_lds_entries(R)];
    __shared__ unsigned wave_count[kDespikeThreads / 64];
    const int t = (int)threadIdx.x;
    unsigned mine = 0;
    for (long long pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        int plane, y0, x0;
        long long tile;
        despike_planes_pair(g, pair, &plane, &tile);
        despike_origin(g, tile, &y0, &x0);
        const T* in = src + (long long)plane * plane_px;
        for (int e = t; e < despike_lds_entries(R); e += kDespikeThreads) win[e] = despike_window_entry<T, R>(in, be, g, y0, x0, e);
        __syncthreads();
        int row, col;
        bool flagged = false;
        if (despike_pixel(g, tile, t, &row, &col)) {
            const long long q = (long long)row * g.W + col;
            T result;
            flagged = despike_replace<T, R>(win, t, despike_load(in, q, be), prm, &result);
            dst[(long long)plane * plane_px + q] = result;
            if (flagged) atomicAdd(events + q, 1);
        }
        mine += (unsigned)__popcll(__ballot(flagged));
        __syncthreads();
    }
    despike_add_count(mine, wave_count, n_flagged);
}

template <typename T, int R>
__global__ __launch_bounds__(kDespikeThreads) void k_despike_planes_sum(const T* __restrict__ src, bool be, bool overlap,
                                                                         DespikeGeom g, long long plane_px, int n_sel,
                                                                         coreg_despike_params prm, bool add_events,
                                                                         double* __restrict__ sum, int* __restrict__ events,
                                                                         unsigned long long* __restrict__ n_flagged) {
    constexpr int entries = despike_lds_entries(R);
    constexpr int slots = despike_planes_stage_slots(R);
    __shared__ double win[2][entries];
    __shared__ unsigned wave_count[kDespikeThreads / 64];
    const int t = (int)threadIdx.x;
    unsigned mine = 0;
    for (long long tile = blockIdx.x; tile < g.items; tile += gridDim.x) {
        int y0, x0, row, col;
        despike_origin(g, tile, &y0, &x0);
        const bool own = despike_pixel(g, tile, t, &row, &col);
        const long long q = own ? (long long)row * g.W + col : 0;
        double acc = 0.0;
        int ev = 0;
        T stored = (T)0;
        if (overlap) {  // plane 0 into the first window
            for (int e = t; e < entries; e += kDespikeThreads) win[0][e] = despike_window_entry<T, R>(src, be, g, y0, x0, e);
            if (own) stored = despike_load(src, q, be);
            __syncthreads();
        }
        for (int k = 0; k < n_sel; ++k) {
            const T* here = src + (long long)k * plane_px;
            const bool more = overlap && k + 1 < n_sel;
            const int cur = overlap ? (k & 1) : 0;
            double next[slots];
            T next_stored = (T)0;
            if (more) {  // plane k + 1 on its way while plane k is decided
#pragma unroll
                for (int s = 0; s < slots; ++s) next[s] = despike_window_entry<T, R>(here + plane_px, be, g, y0, x0, t + s * kDespikeThreads);
                if (own) next_stored = despike_load(here + plane_px, q, be);
            } else if (!overlap) {
                for (int e = t; e < entries; e += kDespikeThreads) win[0][e] = despike_window_entry<T, R>(here, be, g, y0, x0, e);
                if (own) stored = despike_load(here, q, be);
                __syncthreads();
            }
            bool flagged = false;
            if (own) {
                T result;
                flagged = despike_replace<T, R>(win[cur], t, stored, prm, &result);
                acc = despike_planes_add(acc, (double)result);
                ev += flagged ? 1 : 0;
            }
            mine += (unsigned)__popcll(__ballot(flagged));
            if (more) {
#pragma unroll
                for (int s = 0; s < slots; ++s)
                    if (t + s * kDespikeThreads < entries) win[cur ^ 1][t + s * kDespikeThreads] = next[s];
                stored = next_stored;
            }
            __syncthreads();
        }
        if (own) {
            sum[q] = acc;
            events[q] = add_events ? events[q] + ev : ev;
        }
    }
    despike_add_count(mine, wave_count, n_flagged);
}

}  // namespace coreg
