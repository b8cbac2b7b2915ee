// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the mutual-information score of
// the Carrington header-shift sweep -- its edge lists (coreg_sweep_set_bins), the refusals every call sees first, and one
// launch: k_sweep_mi + k_sweep_mi_finalize in place of launch_sweep's k_sweep + k_finalize, over the compacted points of the
// same k_precompute (sweep_mi_plan.hpp plans it; kernels_sweep_mi.hpp has the kernels).
#pragma once
namespace {

MiHave sweep_mi_have(const coreg_handle* h) {
    return MiHave{h->opt_shard_world, (int)h->mi_edges_small.size(), (int)h->mi_edges_large.size()};
}

// the edge lists (csrc/pixels_bins.hpp: 1 to 31 entries, finite, strictly increasing); a refused call leaves the lists set
// before in place
int sweep_mi_set_bins(coreg_handle* h, const double* edges_small, int32_t n_small, const double* edges_large, int32_t n_large) {
    if (!bins_edges_ok(edges_small, n_small) || !bins_edges_ok(edges_large, n_large))
        return fail(h, COREG_EINVAL, "sweep bins: an edge list needs 1 to 31 finite, strictly increasing entries");
    h->mi_edges_small.assign(edges_small, edges_small + n_small);
    h->mi_edges_large.assign(edges_large, edges_large + n_large);
    return COREG_OK;
}

// what a mutual-information sweep is refused for before anything is planned or launched
int check_sweep_mi(coreg_handle* h) {
    const MiPlan p = sweep_mi_admit(sweep_mi_have(h));
    return p.code != COREG_OK ? fail(h, p.code, p.msg) : COREG_OK;
}

// the k_sweep_mi instantiations: the three orders k_refine has, float and double pixels
using SweepMiFn = void (*)(const SweepMiArgs);
int sweep_mi_kernel_index(int order, bool f32) { return (order == 2 ? 0 : (order == 1 ? 1 : 2)) * 2 + (f32 ? 1 : 0); }
SweepMiFn sweep_mi_kernel(int at) {
    static const SweepMiFn table[6] = {k_sweep_mi<2, double>,        k_sweep_mi<2, float>,        k_sweep_mi<1, double>,
                                       k_sweep_mi<1, float>,         k_sweep_mi<ORDER_RT, double>, k_sweep_mi<ORDER_RT, float>};
    return table[at];
}

// One launch: the histograms of the launch's slots, then their scores and counts.  outidx_host: the output indices of the
// launch's slots as the plan holds them (which groups are padding only).
int launch_sweep_mi(coreg_handle* h, const SweepLaunchSpec& L, const long long* outidx_host) {
    const MiPlan p = sweep_mi_plan(MiRequest{sweep_mi_have(h), L.n_slots(), outidx_host, h->opt_mi_chunks});
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);
    HIPCHK(h->mi_hist.reserve((size_t)p.hist_bytes));
    HIPCHK(hipMemsetAsync(h->mi_hist.p, 0, (size_t)p.hist_bytes, h->stream));
    RETCHK(join_small(h));  // the first kernel of the call that reads the image to align

    SweepMiArgs a = {};
    a.img = h->small.p;
    a.W = h->sW;
    a.H = h->sH;
    a.pts = h->pts.as<Pt>();
    a.tile_list = h->tile_list.as<int>();
    a.tile_count = h->tile_count.as<int>();
    a.tile_info = h->tile_info.as<long long>();
    a.lane_params = L.params_dev(h);
    a.out_index = L.outidx_dev(h);
    a.n_slots = L.n_slots();
    a.n_chunks = p.chunks;
    a.order_rt = L.order;
    a.n_small = p.na - 1;
    a.n_large = p.nb - 1;
    std::copy(h->mi_edges_small.begin(), h->mi_edges_small.end(), a.edges_small);
    std::copy(h->mi_edges_large.begin(), h->mi_edges_large.end(), a.edges_large);
    a.hist = h->mi_hist.as<uint32_t>();

    const int at = sweep_mi_kernel_index(L.order, h->small_f32);
    const SweepMiFn fn = sweep_mi_kernel(at);
    if (p.lds_bytes > h->mi_lds[at]) {  // (as host_pixels.hpp does for k_pixels_mi; handles of several threads share the attribute)
        std::lock_guard<std::mutex> lock(g_attr_mutex);
        HIPCHK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
        h->mi_lds[at] = p.lds_bytes;
    }
    EventPair* ev = next_event(h, h->ev_sweep, h->ev_sweep_used);
    if (!ev) return fail(h, COREG_EHIP, "hipEventCreate failed");
    trace("launch_sweep_mi: launching k_sweep_mi");
    HIPCHK(hipEventRecord(ev->a, h->stream));
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(kMiThreads), p.lds_bytes, h->stream, a);
    HIPCHK(hipEventRecord(ev->b, h->stream));
    HIPCHK(hipGetLastError());
    h->stats.n_sweep_launches++;
    h->stats.used_lds = 0;  // (no gather window: the samples come from global memory)

    SweepMiFinalizeArgs f = {};
    f.hist = h->mi_hist.as<uint32_t>();
    f.n_slots = L.n_slots();
    f.n_small = a.n_small;
    f.n_large = a.n_large;
    f.out_index = a.out_index;
    f.lag_begin = L.lag_begin;
    f.out = L.out_dev;
    f.counts = h->counts.as<double>();
    hipLaunchKernelGGL(k_sweep_mi_finalize, dim3((unsigned)L.n_slots()), dim3(kMiFinThreads), 0, h->stream, f);
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

}  // namespace
