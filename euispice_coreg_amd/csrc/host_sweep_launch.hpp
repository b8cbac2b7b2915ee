// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order): one sweep launch, from "the
// plan is on the device" to "coefficients are in out" -- its description (SweepLaunchSpec), the k_sweep variant it runs
// (sweep_variant.hpp) out of the table of instantiations, its fix kernels, k_finalize, and the re-evaluation of flagged
// lag-points or, for a grid-shared sweep, the PendingFinalize that coreg_finalize_sums finishes.
#pragma once
namespace {
using sweep_variant::SweepVariant;
static_assert(sweep_variant::kTranslate == MODE_TRANSLATE && sweep_variant::kHomography == MODE_HOMOGRAPHY &&
                  sweep_variant::kHomographySeries == MODE_HOMOGRAPHY_SERIES && sweep_variant::kCar == MODE_CAR &&
                  sweep_variant::kOrderRt == ORDER_RT, "sweep_variant.hpp restates the kernels' constants");

// One sweep launch: n_batches x kBlock lag slots (padding included) of the uploaded plan, from slot `slot_off` on, over
// the compacted points of the precompute launch before it.
struct SweepLaunchSpec {
    int mode = MODE_TRANSLATE;  // TRANSLATE = Carrington (float64 samples); HOMOGRAPHY[_SERIES], CAR = helioprojective
    int order = 2;
    int method = COREG_METHOD_CORRELATION;
    // first slot in the plan: h->out_index and, in a grid-shared sweep, h->sums count slots; h->lane_params holds one
    // SoA block [2 or 9][n_slots] per launch, one after another
    size_t slot_off = 0;
    int n_batches = 0, n_tiles = 0;
    long long lag_begin = 0;
    double* out_dev = nullptr;
    const LaunchU* car_inv = nullptr;  // MODE_CAR: the launch's native -> pixel map
    const BorderFix* fix = nullptr;    // noise-decided samples of the launch
    int pitch_sel = 0;                 // compile-time LDS window pitch asked for (pick_pitch), 0: per visit
    long long n_slots() const { return (long long)n_batches * kBlock; }
    // both residus methods run the `resid` instantiations of k_sweep; they part in k_finalize (FinalizeArgs.residus)
    bool residus() const { return method != COREG_METHOD_CORRELATION; }
    int residus_kind() const { return method == COREG_METHOD_RESIDUS_MASKED ? 2 : (residus() ? 1 : 0); }
    const double* params_dev(const coreg_handle* h) const {
        return h->lane_params.as<double>() + (mode == MODE_TRANSLATE ? 2 : 9) * slot_off;
    }
    const long long* outidx_dev(const coreg_handle* h) const { return h->out_index.as<long long>() + slot_off; }
};

// ---- the k_sweep variant of a launch ------------------------------------------------------------------------------
struct SweepKernel {
    void (*fn)(const SweepArgs);
    size_t attr_bytes[kMaxDevices];  // per device: the largest dynamic-LDS size the function attribute was raised to
};
template <size_t... I>
SweepKernel* sweep_kernel_table(std::index_sequence<I...>) {
    constexpr const SweepVariant* v = sweep_variant::kSweepVariants.v;
    static SweepKernel table[] = {
        {k_sweep<v[I].mode, v[I].order, std::conditional_t<v[I].f32, float, double>, v[I].round, v[I].resid, v[I].pitch>, {0}}...};
    return table;
}

// per instantiation and device: raise the dynamic-LDS limit once, not per launch (handles of several threads share the
// function attribute, hence the lock)
int raise_dynamic_lds(coreg_handle* h, SweepKernel* k, size_t lds_bytes) {
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    size_t& ab = k->attr_bytes[h->device % kMaxDevices];
    if (lds_bytes > 48 * 1024 && lds_bytes > ab) {
        HIPCHK(hipFuncSetAttribute((const void*)k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        ab = lds_bytes;
    }
    return COREG_OK;
}

// Workgroups of a k_sweep launch of `items` (group, batch) pairs: as many as the device holds at a time -- CUs x the
// workgroups of this instantiation one CU holds at this dynamic-LDS size, the runtime's figure, asked once per (kernel,
// bytes) and handle -- or the "sweep_wgs" option, and never more than there are items; rounded up to a multiple of 8, the
// XCD slots of the item numbering.  (items is a multiple of 8, so the grid never exceeds it.)
int sweep_grid(coreg_handle* h, const SweepKernel* k, size_t lds_bytes, long long items, unsigned* grid) {
    long long resident = h->opt_sweep_wgs;
    if (resident <= 0) {
        if (h->n_cus <= 0) HIPCHK(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->device));
        int per_cu = 0;
        for (const coreg_handle::SweepResidency& r : h->sweep_residency)
            if (r.fn == (const void*)k->fn && r.lds_bytes == lds_bytes) per_cu = r.per_cu;
        if (per_cu <= 0) {
            HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k->fn, kSweepThreads, lds_bytes));
            if (per_cu <= 0) return fail(h, COREG_EHIP, "launch_sweep: the device holds no k_sweep workgroup of this LDS size");
            h->sweep_residency.push_back({(const void*)k->fn, lds_bytes, per_cu});
        }
        resident = (long long)h->n_cus * per_cu;
    }
    *grid = (unsigned)(8 * ((std::min(items, resident) + 7) / 8));
    return COREG_OK;
}

// `a` lacks only the item queue: n_groups8 x 8 groups of this launch, every batch of each
int launch_k_sweep(coreg_handle* h, const SweepLaunchSpec& L, SweepArgs a, int n_groups8, size_t lds_bytes) {
    const SweepVariant v = sweep_variant::pick_sweep_variant(L.mode, L.order, h->small_f32, L.residus(), L.pitch_sel);
    const int at = sweep_variant::sweep_variant_index(v);
    if (at < 0) return fail(h, COREG_EINVAL, "launch_sweep: no k_sweep instantiation for this mode / order / pitch");
    SweepKernel* k = sweep_kernel_table(std::make_index_sequence<sweep_variant::kNumSweepVariants>()) + at;
    EventPair* ev = next_event(h, h->ev_sweep, h->ev_sweep_used);
    if (!ev) return fail(h, COREG_EHIP, "hipEventCreate failed");
    RETCHK(raise_dynamic_lds(h, k, lds_bytes));
    a.items8 = n_groups8 * L.n_batches;
    unsigned grid = 0;
    RETCHK(sweep_grid(h, k, lds_bytes, 8LL * a.items8, &grid));
    // The ticket counters are zeroed before EVERY launch, on the launch's stream: a plate-carree or 5-D sweep launches
    // k_sweep several times behind one k_tile_list, and a launch that failed or a call that was abandoned leaves nothing
    // the next one depends on.  (64 bytes; a base that moves on from launch to launch would save the memset and would
    // have to be kept right across every way a call can end.)
    HIPCHK(h->sweep_queue.reserve(8 * sizeof(unsigned)));
    a.queue = h->sweep_queue.as<unsigned>();
    HIPCHK(hipMemsetAsync(a.queue, 0, 8 * sizeof(unsigned), h->stream));
    HIPCHK(hipEventRecord(ev->a, h->stream));
    hipLaunchKernelGGL(k->fn, dim3(grid), dim3(kSweepThreads), lds_bytes, h->stream, a);
    HIPCHK(hipEventRecord(ev->b, h->stream));
    HIPCHK(hipGetLastError());
    const int rec[7] = {at, v.mode, v.order, v.f32 ? 1 : 0, v.round ? 1 : 0, v.resid ? 1 : 0, v.pitch};
    std::copy(rec, rec + 7, h->last_variant);  // (coreg_last_sweep_variant: a diagnostic, host memory only)
    return COREG_OK;
}

SweepArgs sweep_args(const coreg_handle* h, const SweepLaunchSpec& L, int n_groups, int group_lo, size_t lds_bytes) {
    SweepArgs a;
    a.img = h->small.p;
    a.W = h->sW;
    a.H = h->sH;
    a.pts = h->pts.as<Pt>();
    a.tile_count = h->tile_count.as<int>();
    a.tile_list = h->tile_list.as<int>();
    a.tile_cum = h->tile_cum.as<int>();
    a.group_first = h->group_first.as<int>();
    a.tile_info = h->tile_info.as<long long>();
    a.tile_bbox = h->tile_bbox.as<double>();
    a.visit_rec = h->visit_rec.as<VisitRec>();
    a.lane_params = L.params_dev(h);
    a.n_slots = L.n_slots();
    a.n_batches = L.n_batches;
    a.n_groups = n_groups;
    a.group_lo = group_lo;
    a.partials = h->partials.as<double>();
    a.queue = nullptr;  // (launch_k_sweep)
    a.items8 = 0;
    a.pivots = h->pivots.as<double>();
    a.use_lds = h->opt_use_lds ? 1 : 0;
    a.clean_path = h->opt_clean_path ? 1 : 0;
    a.lds_elems = (int)(lds_bytes / sizeof(double));
    a.car_inv = L.car_inv ? *L.car_inv : LaunchU{};
    a.car_inv.order_rt = L.order;
    a.car_inv.h_incr = (int)h->opt_h_incr;
    return a;
}

// ---- the noise-decided samples of a launch as kernel arguments ------------------------------------------------------
// the fields the three fix kernels' arguments share (BorderFixArgs, ParityFixArgs, TapFixArgs)
template <typename Args>
void fill_fix_common(Args& x, const coreg_handle* h, const SweepLaunchSpec& L) {
    x.img = h->small.p;
    x.W = h->sW;
    x.H = h->sH;
    x.ref = h->ref.p;
    x.ref_f32 = h->ref_dtype == COREG_F32 ? 1 : 0;
    x.gw = h->gW;
    x.order = L.order;
    x.round_f32 = L.mode == MODE_TRANSLATE ? 0 : 1;
    x.residus = L.residus() ? 1 : 0;
    x.pivots = h->pivots.as<double>();
    x.hom = L.params_dev(h);  // SoA [9][n_slots]: the (snapped) map of the slot gives the sample coordinates
    x.n_slots = L.n_slots();
}

// L.fix as FixLaunch: built on every rank of a grid-shared sweep (the re-evaluation of a flagged lag-point runs on every
// rank), run by launch_sweep on the rank that carries the correction
int build_fix_launch(coreg_handle* h, const SweepLaunchSpec& L, FixLaunch* fl) {
    fl->small_f32 = h->small_f32;
    if (!L.fix || !L.fix->any()) return COREG_OK;
    static const std::vector<BorderItems::Item> no_items;
    for (const BorderItems::Item& it : L.fix->border ? L.fix->border->items : no_items) {
        if (it.flags_off >= 0) {
            // odd spline order: re-decide the tap set of every pixel of this lag-point (k_parity_fix), after
            // k_border_fix has set the slab entry (same stream)
            ParityFixArgs p = {};
            fill_fix_common(p, h, L);
            p.flags = h->border_flags.as<unsigned char>() + it.flags_off;
            p.gh = h->gH;
            p.slot = it.slot;
            p.n_partial = 256;
            if (h->fix_partial.reserve((size_t)p.n_partial * kNumSums * sizeof(double)) != hipSuccess)
                return fail(h, COREG_EHIP, "hipMalloc failed (parity fix)");
            p.partial = h->fix_partial.as<double>();
            fl->parity.push_back(p);
        }
        if (it.n == 0) continue;
        BorderFixArgs b = {};
        fill_fix_common(b, h, L);
        b.slot = it.slot;
        b.dropped = h->border_dev.as<int>() + it.first;
        b.n_dropped = it.n;
        fl->border.push_back(b);
    }
    if (L.fix->tap.segs > 0) {
        fl->tap = L.fix->tap;
        fill_fix_common(fl->tap.args, h, L);
    }
    return COREG_OK;
}

// A plate-carree sweep has one launch per combination and every launch lists its single samples anew in the handle's
// buffers: a grid-shared launch's lists are COPIED so that coreg_finalize_sums can run the fix kernels a second time
// about the flagged slots' pivots, as FixLaunch lets it do for the one-launch helioprojective sweeps.  Rare path
// (unrotated maps, single-axis lags).  One allocation, the five lists at 8-byte-rounded offsets; the copies are ordered
// on the handle's stream after the kernels that read the sources, and the next launch's prepare_tap_fix waits for that
// stream before it writes the sources again.
int keep_tap_lists(coreg_handle* h, FixLaunch* fixes) {
    auto kept = std::make_shared<KeptTapLists>();
    const size_t nseg = (size_t)fixes->tap.segs, cnt = (size_t)fixes->tap.count;
    TapFixArgs& t = fixes->tap.args;
    const void* src[5] = {t.xw, t.yw, t.pixel, t.seg_begin, t.seg_slot};
    const size_t bytes[5] = {cnt * sizeof(double), cnt * sizeof(double), cnt * sizeof(unsigned), (nseg + 1) * sizeof(int),
                             nseg * sizeof(int)};
    size_t off[6] = {0};
    for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + ((bytes[k] + 7) & ~(size_t)7);
    HIPCHK(kept->all.reserve(off[5]));
    char* all = kept->all.as<char>();
    for (int k = 0; k < 5; ++k)
        if (bytes[k]) HIPCHK(hipMemcpyAsync(all + off[k], src[k], bytes[k], hipMemcpyDeviceToDevice, h->stream));
    t.xw = (const double*)(all + off[0]);
    t.yw = (const double*)(all + off[1]);
    t.pixel = (const unsigned*)(all + off[2]);
    t.seg_begin = (const int*)(all + off[3]);
    t.seg_slot = (const int*)(all + off[4]);
    fixes->kept = kept;
    return COREG_OK;
}

// A launch of a grid-shared sweep leaves its six sums per slot in h->sums; what coreg_finalize_sums needs to finish it
// from the REDUCED sums is queued here (the extra slab is inside those sums; the second run of the fix kernels happens on
// every rank).
int queue_pending_finalize(coreg_handle* h, const SweepLaunchSpec& L, const RefineArgs& refine, bool refinable,
                           const FixLaunch& fl) {
    coreg_handle::PendingFinalize pf;
    pf.slot_off = (long long)L.slot_off;
    pf.n_slots = L.n_slots();
    pf.lag_begin = L.lag_begin;
    pf.residus = L.residus_kind();
    pf.refine = refine;
    pf.refine.enabled = refinable ? 1 : 0;
    pf.replay_precompute = h->last_precompute;
    pf.fixes = fl;
    if (L.mode == MODE_CAR && fl.tap.segs > 0) RETCHK(keep_tap_lists(h, &pf.fixes));
    h->pending_fin.push_back(pf);
    return COREG_OK;
}

// ---- the launch ---------------------------------------------------------------------------------------------------
int launch_sweep(coreg_handle* h, const SweepLaunchSpec& L) {
    // work space: one slab of six sums per slot and tile group of this launch's share of the grid, one more for the
    // noise-decided samples (a property of the lag-point, not of a share of the grid: rank 0 carries it)
    const long long n_slots = L.n_slots();
    const int n_groups = pick_groups(h, L.n_batches, L.n_tiles);
    const bool sharded = h->opt_shard_world > 1;
    const int g_per = sharded ? n_groups / (int)h->opt_shard_world : n_groups;  // groups swept by this launch
    const int g_lo = sharded ? g_per * (int)h->opt_shard_rank : 0;
    const bool fixing = L.fix && L.fix->any() && (!sharded || h->opt_shard_rank == 0);
    HIPCHK(h->partials.reserve((size_t)(g_per + (fixing ? 1 : 0)) * kNumSums * n_slots * sizeof(double)));
    double* fix_slab = fixing ? h->partials.as<double>() + (size_t)g_per * kNumSums * n_slots : nullptr;
    // the dynamic LDS also carries the end-of-kernel point-group reduction: (kPointGroups-1) x 6 x 256 doubles
    const size_t lds_min = (size_t)(kPointGroups - 1) * kNumSums * kBlock * sizeof(double);
    const size_t lds_bytes = std::max(lds_min, h->opt_use_lds ? (size_t)h->opt_lds_bytes : 0);

    const SweepArgs a = sweep_args(h, L, n_groups, g_lo, lds_bytes);
    RETCHK(join_small(h));  // the first kernel of the call that reads the image to align
    trace("launch_sweep: launching k_sweep");
    if (g_per % 8 != 0) return fail(h, COREG_EINVAL, "launch_sweep: the groups of a launch must be a multiple of 8");
    RETCHK(launch_k_sweep(h, L, a, g_per / 8, lds_bytes));
    h->stats.n_sweep_launches++;
    h->stats.used_lds = a.use_lds;

    FixLaunch fl;
    RETCHK(build_fix_launch(h, L, &fl));
    if (fixing) {
        // the extra slab: zero, except minus the dropped border pixels' totals at the identity lag's slot
        HIPCHK(hipMemsetAsync(fix_slab, 0, (size_t)kNumSums * n_slots * sizeof(double), h->stream));
        RETCHK(launch_fix_kernels(h, fl, fix_slab, nullptr, nullptr));
    }

    // Ill-conditioned lag-points are flagged by k_finalize and re-evaluated about their own means (kernels.hpp:
    // RefineArgs) -- not for the residus methods (another statistic).  A launch with noise-decided samples runs its fix
    // kernels a second time for them (refine.fix_slab: k_finalize only asks whether it is set; refine_with_fixes fills
    // it).  Grid shares across GPUs: the flags can only come from the REDUCED sums, so the re-evaluation is run by
    // coreg_finalize_sums, on every rank, over the whole grid.
    const bool refinable = h->opt_refine && !L.residus();
    FinalizeArgs f = {};
    RETCHK(fill_refine(h, &f.refine, L.mode, L.order, a.lane_params, a.car_inv, n_slots));
    f.refine.enabled = (refinable && !sharded) ? 1 : 0;
    if (fixing && f.refine.enabled) {
        HIPCHK(h->rf_fix_slab.reserve((size_t)kNumSums * n_slots * sizeof(double)));
        f.refine.fix_slab = h->rf_fix_slab.as<double>();
    }
    f.fix_slab = fix_slab;
    f.refine_count = h->counters.as<long long>();  // (null before the first plan: no sweep without one)
    f.partials = h->partials.as<double>();
    f.n_groups = g_per + (fixing ? 1 : 0);
    f.part_stride = n_slots;
    if (sharded) {  // this launch's six sums per slot into h->sums (reserved by the caller for all launches of the sweep)
        f.sums_out = h->sums.as<double>();
        f.sums_stride = h->sums_slots;
        f.sums_off = (long long)L.slot_off;
    }
    f.n_slots = n_slots;
    f.out_index = L.outidx_dev(h);
    f.lag_begin = L.lag_begin;
    f.out = L.out_dev;
    f.counts = h->counts.as<double>();
    f.residus = L.residus_kind();
    f.n_required = (long long)h->gW * h->gH;
    launch_finalize(h, f);
    HIPCHK(hipGetLastError());

    if (sharded) return queue_pending_finalize(h, L, f.refine, refinable, fl);
    if (!f.refine.enabled) return COREG_OK;
    hipLaunchKernelGGL(k_refine_list, dim3(1), dim3(kListThreads), 0, h->stream, f.refine, n_slots, h->counters.as<long long>());
    return refine_with_fixes(h, f.refine, fl, n_slots, f.out_index, L.lag_begin, L.out_dev);
}

}  // namespace
