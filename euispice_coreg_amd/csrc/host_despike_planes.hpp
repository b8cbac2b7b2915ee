// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the planes of a cube despiked
// one by one and summed over the planes (coreg_despike_sum_planes_be) -- the plan
// (csrc/despike_planes_plan.hpp: refusals, geometry; no GPU work), the selected planes up as the file stores them, one
// launch per pass on the handle's stream (csrc/kernels_despike.hpp), the sum, the event map and the counts back.
#pragma once
namespace {

template <typename T>
static void despike_planes_launch_pass(coreg_handle* h, const DespikePlanesPlan& p, const coreg_despike_params& prm, const T* src,
                                       bool be, T* dst, int* events, unsigned long long* count) {
    const auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(p.grid_pairs), dim3(kDespikeThreads), 0, h->stream, src, be, dst, p.g, p.plane_px, p.pairs, prm,
                           events, count);
    };
    if (prm.radius == 1) launch(k_despike_planes_pass<T, 1>);
    else if (prm.radius == 2) launch(k_despike_planes_pass<T, 2>);
    else launch(k_despike_planes_pass<T, 3>);
}

template <typename T>
static void despike_planes_launch_sum(coreg_handle* h, const DespikePlanesPlan& p, const coreg_despike_params& prm, const T* src,
                                      bool be, bool add_events, double* sum, int* events, unsigned long long* count) {
    const bool overlap = h->opt_despike_planes_overlap != 0;
    const auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(p.grid_tiles), dim3(kDespikeThreads), 0, h->stream, src, be, overlap, p.g, p.plane_px, p.n_sel, prm,
                           add_events, sum, events, count);
    };
    if (prm.radius == 1) launch(k_despike_planes_sum<T, 1>);
    else if (prm.radius == 2) launch(k_despike_planes_sum<T, 2>);
    else launch(k_despike_planes_sum<T, 3>);
}

// the passes of a call on the stack at h->dp_raw (big-endian, packed): those before the last write h->dp_a and h->dp_b in
// turn and add their events to the map by atomics; the last one reads what the one before it wrote (the uploaded stack when
// it is the only one) and writes h->dp_sum and h->dp_events
template <typename T>
static int despike_planes_passes(coreg_handle* h, const DespikePlanesPlan& p, const coreg_despike_params& prm) {
    unsigned long long* counts = h->dp_counts.as<unsigned long long>();
    int* events = h->dp_events.as<int>();
    const T* from = h->dp_raw.as<T>();
    bool be = true;
    for (int pass = 0; pass + 1 < prm.n_iter; ++pass) {
        T* to = ((pass & 1) ? h->dp_b : h->dp_a).as<T>();
        despike_planes_launch_pass<T>(h, p, prm, from, be, to, events, counts + pass);
        HIPCHK(hipGetLastError());
        from = to;
        be = false;
    }
    despike_planes_launch_sum<T>(h, p, prm, from, be, prm.n_iter > 1, h->dp_sum.as<double>(), events, counts + prm.n_iter - 1);
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

int despike_sum_planes(coreg_handle* h, const void* base, int32_t bitpix, int64_t plane_stride, int32_t H, int32_t W,
                       const int64_t* plane_index, int32_t n_sel, const coreg_despike_params* prm, double* out_sum,
                       int32_t* out_events, int64_t* n_flagged) {
    const DespikePlanesPlan p = despike_planes_plan(base, bitpix, plane_stride, H, W, plane_index, n_sel, prm, out_sum);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);  // (before any GPU work: a refused call changes nothing)
    const size_t px = (size_t)p.plane_px;
    if (p.n_sel == 0) {  // nothing to sum: no launch
        std::fill(out_sum, out_sum + px, 0.0);
        if (out_events) std::fill(out_events, out_events + px, 0);
        if (n_flagged) std::fill(n_flagged, n_flagged + prm->n_iter, (int64_t)0);
        h->dp_last_ms = 0.0;
        return COREG_OK;
    }
    RETCHK(bind_device_nowait(h));  // (no resident image is read or written: nothing to join)
    const size_t elem = p.f32 ? sizeof(float) : sizeof(double);
    const size_t plane_bytes = px * elem, stack_bytes = plane_bytes * (size_t)p.n_sel;
    HIPCHK(h->dp_pin.reserve(stack_bytes, hipHostMallocDefault, 8));
    HIPCHK(h->dp_raw.reserve(stack_bytes));
    if (prm->n_iter > 1) HIPCHK(h->dp_a.reserve(stack_bytes));
    if (prm->n_iter > 2) HIPCHK(h->dp_b.reserve(stack_bytes));
    HIPCHK(h->dp_sum.reserve(px * sizeof(double)));
    HIPCHK(h->dp_events.reserve(px * sizeof(int)));
    HIPCHK(h->dp_counts.reserve(kDespikeMaxIter * sizeof(unsigned long long)));
    // the selected planes, and of them the rows asked for, packed in the order given (the staging is free: every call waits
    // for its stream before it returns)
    parallel_for(p.n_sel, (unsigned)std::min<size_t>(12, stack_bytes >> 20), 1, [&](long long lo, long long hi) {
        for (long long k = lo; k < hi; ++k)
            std::memcpy((char*)h->dp_pin.p + (size_t)k * plane_bytes,
                        (const char*)base + (size_t)plane_index[k] * (size_t)plane_stride * elem, plane_bytes);
    });
    HIPCHK(hipMemcpyAsync(h->dp_raw.p, h->dp_pin.p, stack_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->dp_counts.p, 0, kDespikeMaxIter * sizeof(unsigned long long), h->stream));
    if (prm->n_iter > 1) HIPCHK(hipMemsetAsync(h->dp_events.p, 0, px * sizeof(int), h->stream));
    if (!h->dp_ev[0].e) {
        HIPCHK(hipEventCreate(&h->dp_ev[0].e));
        HIPCHK(hipEventCreate(&h->dp_ev[1].e));
    }
    HIPCHK(hipEventRecord(h->dp_ev[0], h->stream));
    RETCHK(p.f32 ? despike_planes_passes<float>(h, p, *prm) : despike_planes_passes<double>(h, p, *prm));
    HIPCHK(hipEventRecord(h->dp_ev[1], h->stream));
    HIPCHK(hipMemcpyAsync(out_sum, h->dp_sum.p, px * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_events) HIPCHK(hipMemcpyAsync(out_events, h->dp_events.p, px * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (n_flagged)
        HIPCHK(hipMemcpyAsync(n_flagged, h->dp_counts.p, (size_t)prm->n_iter * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->dp_ev[0], h->dp_ev[1]));
    h->dp_last_ms = ms;
    return COREG_OK;
}

}  // namespace
