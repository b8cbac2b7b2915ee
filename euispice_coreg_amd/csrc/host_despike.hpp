// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): the median/MAD despiking of
// a resident image -- the plan (csrc/despike_plan.hpp: parameter checks, geometry; no GPU work) and one
// launch of k_despike_image (csrc/kernels_despike.hpp) per pass on the handle's stream.
#pragma once
namespace {

// where the flagged counts of a call stand in h->ds_counts (uint64 [2][kDespikeMaxIter]): those of the image to align or of
// a pixel-lag image, read back by the call itself, and those of the last reference preparation, read back on demand
enum DespikeSlot { DESPIKE_SLOT_IMAGE = 0, DESPIKE_SLOT_REFERENCE = 1 };

template <typename T>
static void despike_launch(coreg_handle* h, const DespikePlan& p, const coreg_despike_params& prm, const T* src, T* dst,
                           unsigned long long* count) {
    const auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(p.grid), dim3(kDespikeThreads), 0, h->stream, src, dst, p.g, prm, count);
    };
    if (prm.radius == 1) launch(k_despike_image<T, 1>);
    else if (prm.radius == 2) launch(k_despike_image<T, 2>);
    else launch(k_despike_image<T, 3>);
}

// H x W pixels at `src` (float32 or float64, rows packed; never written) despiked by prm->n_iter passes, each on the result
// of the one before.  The passes write h->ds_a and h->ds_b in turn (buffers of the image's dtype); *last is the one that
// holds the result.  The flagged count of pass i is left at h->ds_counts[slot][i].  Every check comes before any GPU work.
int despike_image(coreg_handle* h, const void* src, bool f32, int H, int W, const coreg_despike_params* prm, DespikeSlot slot,
                  DevBuf** last) {
    const DespikePlan p = despike_plan(H, W, prm);
    if (p.code != COREG_OK) return fail(h, p.code, p.msg);
    const size_t bytes = (size_t)H * W * (f32 ? sizeof(float) : sizeof(double));
    HIPCHK(h->ds_a.reserve(bytes));
    if (prm->n_iter > 1) HIPCHK(h->ds_b.reserve(bytes));
    HIPCHK(h->ds_counts.reserve(2 * kDespikeMaxIter * sizeof(unsigned long long)));
    unsigned long long* counts = h->ds_counts.as<unsigned long long>() + (size_t)slot * kDespikeMaxIter;
    HIPCHK(hipMemsetAsync(counts, 0, kDespikeMaxIter * sizeof(unsigned long long), h->stream));
    const void* from = src;
    for (int pass = 0; pass < prm->n_iter; ++pass) {
        DevBuf* to = (pass & 1) ? &h->ds_b : &h->ds_a;
        if (f32) despike_launch<float>(h, p, *prm, (const float*)from, to->as<float>(), counts + pass);
        else despike_launch<double>(h, p, *prm, (const double*)from, to->as<double>(), counts + pass);
        HIPCHK(hipGetLastError());
        from = to->p;
        *last = to;
    }
    return COREG_OK;
}

// the flagged counts of the last call that used `slot`, out: [n]; waits for the handle's stream
int despike_read_counts(coreg_handle* h, DespikeSlot slot, int n, int64_t* out) {
    HIPCHK(hipMemcpyAsync(out, h->ds_counts.as<unsigned long long>() + (size_t)slot * kDespikeMaxIter, (size_t)n * sizeof(int64_t),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return COREG_OK;
}

}  // namespace
