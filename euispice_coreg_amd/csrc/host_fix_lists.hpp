// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): noise-decided samples, what of their host side uses HIP: the uploads of the plan's border pixels and tap-shift flags (sweep_plan.hpp decides them), the single-sample scan + lists.
#pragma once
namespace {
int upload_border_pixels(coreg_handle* h, const std::vector<int>& pixels) {
    const size_t bytes = std::max<size_t>(1, pixels.size()) * sizeof(int);
    HIPCHK(h->border_dev.reserve(bytes));
    HIPCHK(hipStreamSynchronize(h->stream));  // an earlier sweep may still read the old list / the staging buffer
    HIPCHK(h->pin_border.reserve(bytes));
    std::memcpy(h->pin_border.p, pixels.data(), pixels.size() * sizeof(int));
    if (!pixels.empty())
        HIPCHK(hipMemcpyAsync(h->border_dev.p, h->pin_border.p, pixels.size() * sizeof(int), hipMemcpyHostToDevice,
                              h->stream));
    return COREG_OK;
}

// the tap-shift flags of the noise-decided lag-points (odd orders; one grid each, BorderFix::Item::flags_off)
int upload_border_flags(coreg_handle* h, const std::vector<std::vector<unsigned char>>& flags) {
    if (flags.empty()) return COREG_OK;
    const size_t each = (size_t)h->gW * h->gH;
    HIPCHK(h->border_flags.reserve(each * flags.size()));
    HIPCHK(hipStreamSynchronize(h->stream));  // (pageable source, rare path: blocking copies are fine)
    for (size_t k = 0; k < flags.size(); ++k)
        HIPCHK(hipMemcpy(h->border_flags.as<unsigned char>() + k * each, flags[k].data(), each, hipMemcpyHostToDevice));
    return COREG_OK;
}

// Odd spline orders, general case (kernels.hpp k_tap_scan / k_tap_fix).  Called between the precompute launch (whose
// prologue has put the lag parameters on the device) and the sweep launch: list the (slot, pixel) samples whose mapped
// coordinate lies within 1e-8 px of an integer, evaluate wcslib's chain for them on the host (`shifted_of(slot)` gives the
// slot's shifted header), and leave everything k_tap_fix needs on the device.  The list is sorted (slot, pixel): one
// workgroup per slot adds its entries in a fixed order.  A list beyond "tap_cap" entries (a pure CRVAL1 / CRVAL2 lag set
// under an unrotated header at full size) is not applied at all -- recorded in tap_last, coreg_last_tap_fix.
template <typename ShiftedOf>
// `hom_dev`: the launch's lane parameters (null: the handle's whole buffer); `car_inv` / `car_fwd`: MODE_CAR launches.
int prepare_tap_fix(coreg_handle* h, int sweep_mode, int order, const coreg_wcs2d& target, long long n_slots,
                    const std::vector<unsigned char>& skip, const double box[4], ShiftedOf shifted_of, BorderFix* fix,
                    const double* hom_dev = nullptr, const LaunchU* car_inv = nullptr, const LaunchU* car_fwd = nullptr) {
    // the list starts small (64 K entries, or what an earlier sweep needed) and is grown -- and the scan repeated --
    // only when a sweep lists more, up to "tap_cap"
    const unsigned cap_max = (unsigned)h->opt_tap_cap;
    unsigned cap = (unsigned)std::min<size_t>(cap_max, std::max<size_t>((size_t)1 << 16, h->tap_list.cap / sizeof(uint2)));
    HIPCHK(h->tap_count.reserve(2 * sizeof(unsigned)));  // [0] listed samples, [1] queued segments
    const unsigned seg_cap = 1u << 20;                   // 16 MiB of (slot, row, first, end); beyond: tested in-thread
    HIPCHK(h->tap_segq.reserve((size_t)seg_cap * sizeof(uint4)));
    HIPCHK(h->tap_list.reserve((size_t)cap * sizeof(uint2)));
    HIPCHK(h->tap_skip.reserve((size_t)n_slots));
    HIPCHK(hipMemcpyAsync(h->tap_skip.p, skip.data(), (size_t)n_slots, hipMemcpyHostToDevice, h->stream));
    TapScanArgs a;
    std::memset(&a.cu, 0, sizeof(a.cu));
    std::memset(&a.fwd, 0, sizeof(a.fwd));
    if (car_inv) a.cu = *car_inv;
    if (car_fwd) a.fwd = *car_fwd;
    a.hom = hom_dev ? hom_dev : h->lane_params.as<double>();
    a.n_slots = n_slots;
    a.skip = h->tap_skip.as<unsigned char>();
    a.ref = h->ref.p;
    a.ref_f32 = h->ref_dtype == COREG_F32 ? 1 : 0;
    a.gw = h->gW;
    a.gh = h->gH;
    a.wmax = (double)(h->sW - 1);
    a.hmax = (double)(h->sH - 1);
    a.tol = 1e-8;  // wcslib's round-trip noise stays below 1e-9 px, the homography's below 1e-11
    a.img = h->small.p;
    a.img_f32 = h->small_f32 ? 1 : 0;
    a.W = h->sW;
    a.H = h->sH;
    a.order = order;
    a.nan_filter = (int)h->opt_tap_nan_filter;
    a.bounds_only = (order & 1) ? 0 : 1;
    if (a.bounds_only) a.nan_filter = 0;  // (nothing read from the image to align: no join with its upload either)
    a.seg_list = h->tap_segq.as<uint4>();
    a.seg_count = h->tap_count.as<unsigned>() + 1;
    a.seg_cap = seg_cap;
    if (a.nan_filter) RETCHK(join_small(h));  // (the scan reads the image to align)
    a.count = h->tap_count.as<unsigned>();
    a.list = h->tap_list.as<uint2>();
    a.cap = cap;
    // the sweep's cull box (target pixels that can map into the image for some lag, 3 px of margin): [x0, x1, y0, y1]
    a.i_lo = (int)std::max(0.0, std::min((double)h->gW, box[0]));
    a.i_hi = (int)std::min((double)(h->gW - 1), std::max(-1.0, box[1]));
    a.j_lo = (int)std::max(0.0, std::min((double)h->gH, box[2]));
    a.j_hi = (int)std::min((double)(h->gH - 1), std::max(-1.0, box[3]));
    h->tap_last[0] = h->tap_last[1] = h->tap_last[2] = 0;
    if (a.i_hi < a.i_lo || a.j_hi < a.j_lo) return COREG_OK;
    const int n_rows = a.j_hi - a.j_lo + 1;
    const unsigned gx = (unsigned)((n_slots + 255) / 256);
    const unsigned gy = (unsigned)std::max(1, std::min(n_rows, (int)(4096 / std::max(1u, gx))));
    a.rows_per_block = (n_rows + (int)gy - 1) / (int)gy;
    const dim3 grid(gx, (unsigned)((n_rows + a.rows_per_block - 1) / a.rows_per_block));
    unsigned count = 0;
    for (int pass = 0; pass < 2; ++pass) {
        a.list = h->tap_list.as<uint2>();
        a.cap = cap;
        HIPCHK(hipMemsetAsync(h->tap_count.p, 0, 2 * sizeof(unsigned), h->stream));
        if (sweep_mode == MODE_CAR) {
            hipLaunchKernelGGL((k_tap_scan<MODE_CAR>), grid, dim3(256), 0, h->stream, a);
            hipLaunchKernelGGL((k_tap_scan_segments<MODE_CAR>), dim3(2048), dim3(256), 0, h->stream, a);
        } else if (sweep_mode == MODE_HOMOGRAPHY_SERIES) {
            hipLaunchKernelGGL((k_tap_scan<MODE_HOMOGRAPHY_SERIES>), grid, dim3(256), 0, h->stream, a);
            hipLaunchKernelGGL((k_tap_scan_segments<MODE_HOMOGRAPHY_SERIES>), dim3(2048), dim3(256), 0, h->stream, a);
        } else {
            hipLaunchKernelGGL((k_tap_scan<MODE_HOMOGRAPHY>), grid, dim3(256), 0, h->stream, a);
            hipLaunchKernelGGL((k_tap_scan_segments<MODE_HOMOGRAPHY>), dim3(2048), dim3(256), 0, h->stream, a);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&count, h->tap_count.p, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (count <= cap || count > cap_max) break;
        cap = count;  // (the scan is deterministic in what it lists: the second pass finds exactly `count` entries)
        HIPCHK(h->tap_list.reserve((size_t)cap * sizeof(uint2)));
    }
    h->tap_last[0] = count;
    h->tap_last[1] = 0;
    h->tap_last[2] = count > cap ? 1 : 0;
    if (count == 0 || count > cap) return COREG_OK;
    // the scan's list back; grouped by slot, put in pixel order and evaluated with wcslib's chain on the host
    // (sweep_plan.hpp group_tap_samples); the lists k_tap_fix reads up
    static_assert(sizeof(TapSample) == sizeof(uint2), "TapSample mirrors the uint2 entries of k_tap_scan's list");
    std::vector<TapSample> list(count);
    HIPCHK(hipMemcpy(list.data(), h->tap_list.p, (size_t)count * sizeof(uint2), hipMemcpyDeviceToHost));
    const TapLists t = group_tap_samples(list, n_slots, h->gW, target, shifted_of);
    const int n_seg = (int)t.seg_slot.size();
    HIPCHK(h->tap_seg_slot.reserve((size_t)n_seg * sizeof(int)));
    HIPCHK(h->tap_seg_begin.reserve((size_t)(n_seg + 1) * sizeof(int)));
    HIPCHK(h->tap_pixel.reserve((size_t)count * sizeof(unsigned)));
    HIPCHK(h->tap_xw.reserve((size_t)count * sizeof(double)));
    HIPCHK(h->tap_yw.reserve((size_t)count * sizeof(double)));
    // (pageable sources, rare path: blocking copies)
    HIPCHK(hipMemcpy(h->tap_seg_slot.p, t.seg_slot.data(), (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tap_seg_begin.p, t.seg_begin.data(), (size_t)(n_seg + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tap_pixel.p, t.pixel.data(), (size_t)count * sizeof(unsigned), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tap_xw.p, t.xw.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tap_yw.p, t.yw.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    fix->tap.segs = n_seg;
    fix->tap.count = (long long)count;
    fix->tap.mode = sweep_mode;
    fix->tap.args.seg_slot = h->tap_seg_slot.as<int>();
    fix->tap.args.seg_begin = h->tap_seg_begin.as<int>();
    fix->tap.args.pixel = h->tap_pixel.as<unsigned>();
    fix->tap.args.xw = h->tap_xw.as<double>();
    fix->tap.args.yw = h->tap_yw.as<double>();
    fix->tap.args.cu = a.cu;
    fix->tap.args.fwd = a.fwd;
    h->tap_last[1] = n_seg;
    return COREG_OK;
}

}  // namespace
