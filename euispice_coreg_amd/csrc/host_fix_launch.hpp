// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): noise-decided samples
// (DESIGN 4b), launch side: the fixes of a launch as the planner leaves them (BorderFix), work space of the re-evaluation,
// the one k_finalize launch, the fix kernels of one launch, and their second run with k_refine.
#pragma once
namespace {
struct BorderFix {  // the noise-decided samples of a launch
    // lag-points whose border pixels are decided by wcslib's rounding noise: the plan's (sweep_plan.hpp; its pixels are in
    // h->border_dev, its flag grids in h->border_flags), or none
    const BorderItems* border = nullptr;
    TapFix tap;  // single samples near an integer coordinate (odd spline orders): device arrays ready for k_tap_fix
    bool any() const { return (border && !border->items.empty()) || tap.segs > 0; }
};

// work space + arguments of the re-evaluation of ill-conditioned lag-points (kernels.hpp: RefineArgs) for a launch of
// n_slots lag slots whose parameters are at params_dev
int fill_refine(coreg_handle* h, RefineArgs* r, int mode, int order, const double* params_dev, const LaunchU& car_inv,
                long long n_slots) {
    HIPCHK(h->rf_flags.reserve((size_t)n_slots * sizeof(int)));
    HIPCHK(h->rf_pivots.reserve((size_t)n_slots * 2 * sizeof(double)));
    HIPCHK(h->rf_list.reserve((size_t)n_slots * sizeof(int)));
    if (!h->rf_head.p) {
        HIPCHK(h->rf_head.reserve(4 * sizeof(int)));
        HIPCHK(hipMemsetAsync(h->rf_head.p, 0, 4 * sizeof(int), h->stream));  // (the two tickets start at zero)
    }
    // work items: (flagged slots) x (chunks per slot) <= max(kRefineItems, n_slots), see refine_list_block
    HIPCHK(h->rf_partial.reserve((size_t)std::max<long long>(kRefineItems, n_slots) * kNumSums * sizeof(double)));
    std::memset(r, 0, sizeof(*r));
    r->cond = std::pow(10.0, (double)h->opt_refine_cond_log10);
    r->mode = mode;
    r->order = order;
    r->small_f32 = h->small_f32 ? 1 : 0;
    r->img = h->small.p;
    r->W = h->sW;
    r->H = h->sH;
    r->pts = h->pts.as<Pt>();
    r->tile_list = h->tile_list.as<int>();
    r->tile_count = h->tile_count.as<int>();
    r->tile_info = h->tile_info.as<long long>();
    r->lane_params = params_dev;
    r->pivots = h->pivots.as<double>();
    r->car_inv = car_inv;
    r->flags = h->rf_flags.as<int>();
    r->slot_pivots = h->rf_pivots.as<double>();
    r->list = h->rf_list.as<int>();
    r->head = h->rf_head.as<int>();
    r->partial = h->rf_partial.as<double>();
    return COREG_OK;
}

// k_finalize over the n_slots lag slots of `f`: the one place that knows its launch geometry
void launch_finalize(coreg_handle* h, const FinalizeArgs& f) {
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((f.n_slots + kFinSlots - 1) / kFinSlots)), dim3(kFinThreads), 0, h->stream, f);
}

// fn(TS()) with TS the element type of the image to align (float or double), as context_types
template <typename Fn>
void with_pixel_type(bool f32, Fn fn) {
    if (f32) fn(float());
    else fn(double());
}

// the fix kernels of one launch (FixLaunch) into `slab`; slot_pivots / only_flagged: the second run (kernels.hpp:
// BorderFixArgs)
int launch_fix_kernels(coreg_handle* h, const FixLaunch& fl, double* slab, const double* slot_pivots, const int* only_flagged) {
    auto second_run = [&](auto args) {
        args.slab = slab;
        args.slot_pivots = slot_pivots;
        args.only_flagged = only_flagged;
        return args;
    };
    with_pixel_type(fl.small_f32, [&](auto ts) {
        using TS = decltype(ts);
        for (const BorderFixArgs& b : fl.border)
            hipLaunchKernelGGL((k_border_fix<TS>), dim3(1), dim3(256), 0, h->stream, second_run(b));
        for (const ParityFixArgs& p0 : fl.parity) {
            const ParityFixArgs p = second_run(p0);
            hipLaunchKernelGGL((k_parity_fix<TS>), dim3(p.n_partial), dim3(256), 0, h->stream, p);
            hipLaunchKernelGGL(k_parity_fix_final, dim3(1), dim3(64), 0, h->stream, p);
        }
        if (fl.tap.segs > 0) {
            const TapFixArgs t = second_run(fl.tap.args);
            const dim3 tg((unsigned)fl.tap.segs), tb(256);
            if (fl.tap.mode == MODE_CAR) hipLaunchKernelGGL((k_tap_fix<TS, MODE_CAR>), tg, tb, 0, h->stream, t);
            else if (fl.tap.mode == MODE_HOMOGRAPHY_SERIES)
                hipLaunchKernelGGL((k_tap_fix<TS, MODE_HOMOGRAPHY_SERIES>), tg, tb, 0, h->stream, t);
            else hipLaunchKernelGGL((k_tap_fix<TS, MODE_HOMOGRAPHY>), tg, tb, 0, h->stream, t);
        }
    });
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

// After a k_finalize that has written the flags and a k_refine_list that has listed the flagged slots: the launch's
// noise-decided samples (if it has any) about the flagged slots' OWN pivots into a slab of their own (kernels that leave
// at once unless the slot is flagged), then k_refine re-evaluates the listed slots, adds that slab and overwrites their
// coefficients (its last block).  No host round trip; with nothing flagged (the normal case) every block leaves at once.
// launch_sweep on one GPU, coreg_finalize_sums on every rank of a grid-shared sweep.
int refine_with_fixes(coreg_handle* h, RefineArgs r, const FixLaunch& fixes, long long n_slots,
                      const long long* outidx_dev, long long lag_begin, double* out_dev) {
    if (!fixes.empty()) {
        const size_t bytes = (size_t)kNumSums * n_slots * sizeof(double);
        HIPCHK(h->rf_fix_slab.reserve(bytes));
        HIPCHK(hipMemsetAsync(h->rf_fix_slab.p, 0, bytes, h->stream));
        r.fix_slab = h->rf_fix_slab.as<double>();
        RETCHK(launch_fix_kernels(h, fixes, h->rf_fix_slab.as<double>(), r.slot_pivots, r.flags));
    }
    r.out_index = outidx_dev;
    r.lag_begin = lag_begin;
    r.out = out_dev;
    r.counts = h->counts.as<double>();
    hipLaunchKernelGGL(k_refine, dim3(kRefineBlocks), dim3(kRefineThreads), 0, h->stream, r, n_slots);
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

}  // namespace
