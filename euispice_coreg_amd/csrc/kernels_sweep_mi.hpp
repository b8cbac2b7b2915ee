// Part of csrc/kernels.hpp: the mutual-information score of the Carrington header-shift sweep (coreg_sweep_carrington with
// COREG_METHOD_MUTUAL_INFORMATION).
//
//   k_sweep_mi<ORDER, TS>  MODE_TRANSLATE only.  One workgroup per (group of kMiG = 16 lag slots, chunk of the launch's tile
//                          list), walked like k_refine's work items: per compacted point one Pt, per slot the coordinates
//                          x0[slot] + b0, y0[slot] + b1 and the sample from global memory (L2) through the per-point spline
//                          path of kernels_common.hpp -- the coordinates, bounds rule, mirrored taps and NaN poisoning of
//                          the Pearson sweep's per-point path.  A kept pair (the reference value is finite: k_precompute
//                          drops the others; the sample is in bounds and finite) adds 1 to the cell (bin of the sample among
//                          edges_small, bin of the reference value among edges_large) of its slot's histogram.  The RAW
//                          values are binned: the launch's precompute leaves the reference value as stored in Pt.a (its
//                          `residus` layout), the sample is the interpolated value, no pivot is subtracted anywhere.
//                          The histograms are uint32 counters in LDS, [cell][slot]: a wave-instruction takes 4 points x 16
//                          slots, and the sixteen lanes of a point hit sixteen neighbouring dwords (the layout
//                          kernels_pixels_mi.hpp measured against the alternative).  A padding slot has NaN parameters,
//                          fails the bounds rule and adds nothing; a group of padding slots only leaves at once.  When the
//                          walk is done the non-zero cells are added to the launch's global histograms, uint32
//                          [slot][cell], with integer atomicAdd: the result does not depend on the order of the adds, hence
//                          not on the chunks, the groups, the batch or the slot a lag-point was given.
//   k_sweep_mi_finalize    one workgroup per lag slot: margins, the terms row by row and the score in the fixed order of
//                          csrc/pixels_bins.hpp; writes out[out_index[slot] - lag_begin] and counts[...] as k_finalize does
//                          and skips the slots whose out_index is negative.
//
// LDS: the histograms are dynamic, kMiG * na * nb * 4 bytes (64 KiB at 32 x 32 bins, 16 KiB at 16 x 16); the two edge lists
// are static.  No floating-point atomic anywhere.
#pragma once
#include "pixels_bins.hpp"
#include "sweep_mi_plan.hpp"
namespace coreg {

static_assert(kMiMaxEdges == kPixMaxEdges, "sweep_mi_plan.hpp restates the edge limit of pixels_bins.hpp");
static_assert(kMiThreads % kMiG == 0 && (kMiG & (kMiG - 1)) == 0, "threads = points per step x slots, slots a power of two");

struct SweepMiArgs {
    const void* img;  // image to align, float / double [H][W]
    int W, H;
    const Pt* pts;
    const int* tile_list;
    const int* tile_count;
    const long long* tile_info;
    const double* lane_params;   // SoA [2][n_slots]: X0, Y0 of the launch's slots
    const long long* out_index;  // [n_slots]
    long long n_slots;
    int n_chunks;
    int order_rt;  // the spline order (read by the ORDER_RT instantiation)
    int n_small, n_large;
    double edges_small[kMiMaxEdges], edges_large[kMiMaxEdges];
    uint32_t* hist;  // [n_slots][na * nb], zero at launch
};

template <int ORDER, typename TS>
__global__ __launch_bounds__(kMiThreads) void k_sweep_mi(const SweepMiArgs a) {
    extern __shared__ uint32_t mi_hist[];  // [na * nb][kMiG]
    __shared__ double mi_edges[2][kMiMaxEdges];
    const int tid = threadIdx.x;
    const int group = (int)blockIdx.x / a.n_chunks, chunk = (int)blockIdx.x - group * a.n_chunks;
    const int slot = tid & (kMiG - 1), sub = tid >> 4;
    const long long gslot = (long long)group * kMiG + slot;  // (< n_slots: the grid is n_slots / kMiG groups)
    if (!__syncthreads_or(tid < kMiG && a.out_index[gslot] >= 0)) return;  // padding only (uniform)
    const int na = a.n_small + 1, nb = a.n_large + 1, n_cells = na * nb;
    for (int q = tid; q < n_cells * kMiG; q += kMiThreads) mi_hist[q] = 0u;
    if (tid < a.n_small) mi_edges[0][tid] = a.edges_small[tid];
    if (tid >= 64 && tid - 64 < a.n_large) mi_edges[1][tid - 64] = a.edges_large[tid - 64];
    __syncthreads();

    const TS* __restrict__ img = (const TS*)a.img;
    const double x0 = a.lane_params[gslot], y0 = a.lane_params[a.n_slots + gslot];
    const int n_list = (int)a.tile_info[0];
    for (int tl = mi_chunk_first(chunk, a.n_chunks); tl < n_list; tl += mi_chunk_step(a.n_chunks)) {
        const int tile = a.tile_list[tl];
        const int cnt = a.tile_count[tile];
        const Pt* __restrict__ pts = a.pts + (size_t)tile * kTilePts;
        for (int p = sub; p < cnt; p += kMiThreads / kMiG) {
            const Pt pt = pts[p];
            const double nx = x0 + pt.b0, ny = y0 + pt.b1;  // self.x + term, utils/rectify.py:362 (point_lag)
            bool inb;
            double v;
            if constexpr (ORDER == ORDER_RT) v = spline_global_rt<TS>(img, a.W, a.H, nx, ny, a.order_rt, inb);
            else v = spline_global<ORDER, TS>(img, a.W, a.H, nx, ny, inb);
            if (inb && isfinite(v)) {
                const int i = bins_index(mi_edges[0], a.n_small, v);
                const int j = bins_index(mi_edges[1], a.n_large, pt.a);
                atomicAdd(&mi_hist[(i * nb + j) * kMiG + slot], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* __restrict__ gh = a.hist + (size_t)group * kMiG * n_cells;
    for (int q = tid; q < n_cells * kMiG; q += kMiThreads) {
        const uint32_t v = mi_hist[q];
        if (v) atomicAdd(&gh[(size_t)(q & (kMiG - 1)) * n_cells + (q >> 4)], v);
    }
}

struct SweepMiFinalizeArgs {
    const uint32_t* hist;  // [n_slots][na * nb]
    long long n_slots;
    int n_small, n_large;
    const long long* out_index;  // C-order raveled lag index of each slot, or -1 (padding)
    long long lag_begin;
    double* out;     // [lag_end - lag_begin]
    double* counts;  // the same: the pairs in the lag-point's histogram
};
constexpr int kMiFinThreads = 64;

__global__ __launch_bounds__(kMiFinThreads) void k_sweep_mi_finalize(const SweepMiFinalizeArgs a) {
    __shared__ uint32_t s_r[kMiMaxEdges + 1], s_c[kMiMaxEdges + 1];
    __shared__ double s_rows[kMiMaxEdges + 1];
    const long long slot = blockIdx.x;
    const long long idx = a.out_index[slot];
    if (idx < 0) return;  // (uniform)
    const int tid = threadIdx.x;
    const int na = a.n_small + 1, nb = a.n_large + 1;
    const uint32_t* __restrict__ h = a.hist + (size_t)slot * na * nb;
    // margins: threads [0, na) a row each, threads [32, 32 + nb) a column each
    if (tid < na) {
        uint32_t v = 0;
        for (int j = 0; j < nb; ++j) v += h[tid * nb + j];
        s_r[tid] = v;
    } else if (tid >= 32 && tid - 32 < nb) {
        uint32_t v = 0;
        for (int i = 0; i < na; ++i) v += h[i * nb + (tid - 32)];
        s_c[tid - 32] = v;
    }
    __syncthreads();
    uint32_t n = 0;
    for (int i = 0; i < na; ++i) n += s_r[i];
    // the terms of a row in the order of j: one thread per row
    if (tid < na) s_rows[tid] = n > 0 ? bins_mi_row(h, 1, tid, nb, s_r[tid], s_c, 1, n) : 0.0;
    __syncthreads();
    if (tid == 0) {
        a.out[idx - a.lag_begin] = bins_mi_sum(s_rows, 1, na, n);
        a.counts[idx - a.lag_begin] = (double)n;
    }
}

}  // namespace coreg
