// The plan of coreg_despike_sum_planes_be: a stack of planes [n_sel][H][W], every plane
// despiked on its own by the rule of despike_plan.hpp, then summed over the planes in float64.  Here: the refusals with
// their code and message, the launch geometry -- the tiles of despike_plan.hpp; the passes before the last one deal (plane,
// tile) pairs, the last pass deals tiles and walks the planes in order -- and the one addition of the sum.  Plain C++ with
// no HIP dependency: included by kernels_despike.hpp and by the host parts of libcoreg_hip.so's one translation
// unit; tests/native/despike_planes_rules.cpp walks it on the host under sanitizers.
#pragma once
#include "despike_plan.hpp"

namespace coreg {

constexpr int kDespikePlanesMaxSel = 4096;  // planes of a call at most

// sum[j,i] = add(... add(add(+0.0, v[0,j,i]), v[1,j,i]) ..., v[n_sel-1,j,i]): a NaN is a +0.0 term, +-Inf pass through (as
// np.nansum); one float64 addition per plane, in the order of the planes
COREG_DS_HD double despike_planes_add(double acc, double v) { return acc + (v != v ? 0.0 : v); }

// the work items of a pass before the last: pair = plane * g.items + tile
COREG_DS_HD void despike_planes_pair(const DespikeGeom& g, long long pair, int* plane, long long* tile) {
    *plane = (int)(pair / g.items);
    *tile = pair % g.items;
}

// the window entries a thread stages per plane: entries t, t + kDespikeThreads, ... below despike_lds_entries(R)
COREG_DS_HD constexpr int despike_planes_stage_slots(int R) {
    return (despike_lds_entries(R) + kDespikeThreads - 1) / kDespikeThreads;
}

// A refusal (code != COREG_OK, msg) or what the launches of a call need
struct DespikePlanesPlan {
    int code = COREG_OK;
    const char* msg = nullptr;
    DespikeGeom g = {};      // of one plane
    int n_sel = 0;           // 0: no launch; the sum is +0.0 everywhere, no events, no counts
    bool f32 = false;        // BITPIX -32
    long long plane_px = 0;  // H x W: elements between two planes of the packed stack on the device
    long long pairs = 0;     // n_sel x g.items: work items of a pass before the last
    unsigned grid_pairs = 0; // workgroups of such a pass: min(pairs, kDespikeMaxGrid)
    unsigned grid_tiles = 0; // workgroups of the last pass: min(g.items, kDespikeMaxGrid)
    size_t lds = 0;          // LDS of a workgroup of the last pass: two windows (the next plane is staged under the current one)
};

inline DespikePlanesPlan despike_planes_plan(const void* base, int bitpix, long long plane_stride, long long H, long long W,
                                             const int64_t* plane_index, long long n_sel, const coreg_despike_params* prm,
                                             const void* out_sum) {
    DespikePlanesPlan p;
    const char* why = despike_params_refusal(prm);
    if (!why && bitpix != -32 && bitpix != -64) why = "despike_sum_planes: BITPIX must be -32 or -64";
    if (!why && (H < 1 || W < 1 || H > 2147483647ll / W)) why = "despike_sum_planes: empty plane, or more than 2^31 - 1 pixels";
    if (!why && plane_stride < H * W) why = "despike_sum_planes: plane_stride is below H x W";
    if (!why && (n_sel < 0 || n_sel > kDespikePlanesMaxSel)) why = "despike_sum_planes: n_sel must be from 0 to 4096";
    if (!why && (!base || !out_sum || (n_sel > 0 && !plane_index))) why = "despike_sum_planes: null pointer";
    if (!why)
        for (long long k = 0; k < n_sel; ++k)
            if (plane_index[k] < 0) why = "despike_sum_planes: negative plane index";
    if (why) {
        p.code = COREG_EINVAL;
        p.msg = why;
        return p;
    }
    p.g = despike_plan(H, W, prm).g;
    p.n_sel = (int)n_sel;
    p.f32 = bitpix == -32;
    p.plane_px = H * W;
    p.pairs = n_sel * p.g.items;
    p.grid_pairs = (unsigned)std::min(p.pairs, kDespikeMaxGrid);
    p.grid_tiles = (unsigned)std::min(p.g.items, kDespikeMaxGrid);
    p.lds = 2 * despike_lds_bytes(prm->radius);
    return p;
}

}  // namespace coreg
