// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): planning of a sweep: lag dimensions and checks, tile shape + lag patch, lag slots, tile groups, precompute launch, LDS pitch.
#pragma once
namespace {
// ---- host fork/join ---------------------------------------------------------------------------------------------
// fn(lo, hi) over [0, n) in chunks of `grain` items (0: one even share per thread) dealt from a shared counter, on up to
// `max_threads` threads, this one included, and never more than there are chunks or cores.  Every caller's items are
// independent of one another, so the split never changes a result.  Work run here must not touch the handle's caches.
template <typename Fn>
void parallel_for(long long n, unsigned max_threads, long long grain, Fn fn) {
    if (n <= 0) return;
    const long long nt_max = std::max<long long>(1, std::min(max_threads, std::thread::hardware_concurrency()));
    if (grain <= 0) grain = (n + nt_max - 1) / nt_max;
    const long long nt = std::min(nt_max, (n + grain - 1) / grain);
    if (nt <= 1) {
        fn(0ll, n);
        return;
    }
    std::atomic<long long> next(0);
    auto worker = [&] {
        for (long long lo = next.fetch_add(grain); lo < n; lo = next.fetch_add(grain)) fn(lo, std::min(n, lo + grain));
    };
    std::vector<std::thread> th;
    for (long long t = 1; t < nt; ++t) th.emplace_back(worker);
    worker();
    for (auto& x : th) x.join();
}

// ---- lag batching (lag_plan.hpp: the planner and the slot layout, plain C++) ------------------------------------------
using lag_plan::Geometry;
using lag_plan::LagDims;
using lag_plan::Plan;
using lag_plan::SlotList;
using lag_plan::build_slots;
static_assert(lag_plan::kSlots == kBlock && lag_plan::kWaveLags == 64, "lag_plan.hpp restates the kernels' constants");

// The one-shot combination range ("combo_begin" / "combo_end") belongs to THE NEXT sweep call, whatever becomes of it: the
// entry points take it off the handle before any validation (a call that failed early used to leave it armed
// for an unrelated later sweep) and hand it to check_lags.
struct ComboRange {
    long long begin = 0, end = 0;
};
ComboRange take_combo_range(coreg_handle* h) {
    ComboRange r;
    r.begin = h->opt_combo_begin;
    r.end = h->opt_combo_end;
    h->opt_combo_begin = h->opt_combo_end = 0;
    return r;
}
int check_lags(coreg_handle* h, const coreg_lags* l, LagDims* d, int64_t begin, int64_t end, ComboRange combo = ComboRange()) {
    if (!l || !l->crval1 || !l->crval2 || !l->cdelt1 || !l->cdelt2 || !l->crota)
        return fail(h, COREG_EINVAL, "lags: null array");
    if (l->n_crval1 < 1 || l->n_crval2 < 1 || l->n_cdelt1 < 1 || l->n_cdelt2 < 1 || l->n_crota < 1)
        return fail(h, COREG_EINVAL, "lags: every axis needs at least one value");
    d->n1 = l->n_crval1;
    d->n2 = l->n_crval2;
    d->n3 = l->n_cdelt1;
    d->n4 = l->n_cdelt2;
    d->n5 = l->n_crota;
    d->nc = (long long)d->n3 * d->n4 * d->n5;
    d->c0 = 0;
    {
        // one-shot combination range of a multi-GPU sweep (taken off the handle by the entry point)
        const long long cb = combo.begin, ce = combo.end;
        if (cb != 0 || ce != 0) {
            if (cb < 0 || ce <= cb || ce > d->nc)
                return fail(h, COREG_EINVAL, "combo_begin/combo_end outside [0, n_cdelt1 * n_cdelt2 * n_crota]");
            d->c0 = cb;
            d->nc = ce - cb;
        }
    }
    if (begin < 0 || end > d->total() || begin > end)
        return fail(h, COREG_EINVAL, "lag_begin/lag_end outside [0, n_lags]");
    const double* ax[5] = {l->crval1, l->crval2, l->cdelt1, l->cdelt2, l->crota};
    const int32_t na[5] = {l->n_crval1, l->n_crval2, l->n_cdelt1, l->n_cdelt2, l->n_crota};
    for (int k = 0; k < 5; ++k)
        for (int32_t i = 0; i < na[k]; ++i)
            if (!std::isfinite(ax[k][i])) return fail(h, COREG_EINVAL, "lags: a non-finite value");
    return COREG_OK;
}

// Headers / grids that cannot give finite pixel coordinates are refused before anything is planned or launched
// (geometry.hpp wcs_problem: the reference would hand such a header to astropy, which raises, or return NaN everywhere).
static int check_wcs(coreg_handle* h, const coreg_wcs2d* w, bool carrington_transform) {
    const char* why = wcs_problem(*w, carrington_transform);
    return why ? fail(h, COREG_EINVAL, why) : COREG_OK;
}
// Pixel and grid-point counts are 32-bit in the kernels' lists (active points, border pixels, tiles): refuse what does not fit.
static int check_grid(coreg_handle* h, const coreg_carr_grid* g) {
    if (g->n_lon >= 1 && g->n_lat >= 1 && too_many(g->n_lon, g->n_lat))
        return fail(h, COREG_EINVAL, "Carrington grid: more than 2^31 - 1 points");
    const char* why = grid_problem(*g);
    return why ? fail(h, COREG_EINVAL, why) : COREG_OK;
}

// Tile shape and lag patches of a sweep (lag_plan::plan_patches) under the handle's options.  m1 x n2 = lag plane.
Plan choose_plan(coreg_handle* h, const Geometry& g, int m1, int n2, long long lds_elems) {
    lag_plan::PlanOptions o;
    o.tile_w = (int)h->opt_tile_w;
    o.patch_w = (int)h->opt_patch_w;
    coreg_handle::PlanMemo& memo = h->plan_memo;
    const bool same = memo.valid && memo.m1 == m1 && memo.n2 == n2 && memo.lds_elems == lds_elems && memo.o.tile_w == o.tile_w &&
                      memo.o.patch_w == o.patch_w && std::memcmp(&memo.g, &g, sizeof(g)) == 0;
    if (!same) {
        memo.plan = lag_plan::plan_patches(g, m1, n2, lds_elems, o, kTilePts);
        memo.g = g;
        memo.m1 = m1;
        memo.n2 = n2;
        memo.lds_elems = lds_elems;
        memo.o = o;
        memo.valid = true;
    }
    const Plan& r = memo.plan;
    if (std::getenv("COREG_DEBUG_PLAN")) {
        std::string patches;
        for (size_t k = 0; k < r.rects.size(); ++k) {
            size_t n = 1;
            while (k + n < r.rects.size() && r.rects[k + n].w == r.rects[k].w && r.rects[k + n].h == r.rects[k].h) ++n;
            patches += (patches.empty() ? "" : " + ") + std::to_string(n) + " of " + std::to_string(r.rects[k].w) + " x " +
                       std::to_string(r.rects[k].h);
            k += n - 1;
        }
        std::fprintf(stderr, "[coreg plan] tile %d x %d, lag patches %s = %d live lag-waves, window estimate %.0f (%.1f x %.1f) of %lld elements; "
                     "geometry d/di (%.3f, %.3f) d/dj (%.3f, %.3f) lag1 (%.3f, %.3f) lag2 (%.3f, %.3f)\n", r.tile_w,
                     kTilePts / r.tile_w, patches.c_str(), r.live_waves, r.window, r.win_w, r.win_h, lds_elems, g.dx_di, g.dy_di,
                     g.dx_dj, g.dy_dj, g.ax, g.ay, g.bx, g.by);
    }
    return r;
}

// indices of the smallest, the most central and the largest value of a lag axis (any order, NaNs ignored)
void extreme_lags(const double* v, int n, int out[3]) {
    int lo = 0, hi = 0;
    for (int i = 1; i < n; ++i) {
        if (v[i] < v[lo] || v[lo] != v[lo]) lo = i;
        if (v[i] > v[hi] || v[hi] != v[hi]) hi = i;
    }
    const double mid = 0.5 * (v[lo] + v[hi]);
    int m = lo;
    for (int i = 0; i < n; ++i)
        if (std::fabs(v[i] - mid) < std::fabs(v[m] - mid)) m = i;
    out[0] = lo;
    out[1] = m;
    out[2] = hi;
}

// mean spacing of a lag axis over its value range (plan heuristics only; lists may come in any order)
double lag_step(const double* v, int n) {
    if (n < 2) return 0.0;
    double lo = v[0], hi = v[0];
    for (int i = 1; i < n; ++i) {
        lo = std::min(lo, v[i]);
        hi = std::max(hi, v[i]);
    }
    return (hi - lo) / (double)(n - 1);
}

int pick_groups(coreg_handle* h, int n_batches, int n_tiles) {
    // the compacted points are cut in n_groups EQUAL shares (k_tile_list), so n_groups * n_batches workgroups of equal
    // work: 256 groups make every round of 256 CUs full; fewer when there are many lag batches
    if (h->opt_shard_world > 1) {
        // point sharding: every rank takes a multiple of 8 groups (the XCD-aware block mapping of k_sweep), as close
        // to one full round of 256 workgroups as the batch count allows
        const long long per_rank = 8 * std::max<long long>(1, std::llround(256.0 / (8.0 * n_batches)));
        return (int)std::min<long long>(per_rank * h->opt_shard_world, 1000 / (8 * h->opt_shard_world) * 8 * h->opt_shard_world);
    }
    long long g = h->opt_n_groups > 0 ? h->opt_n_groups : (4096 + n_batches - 1) / n_batches;
    (void)n_tiles;
    g = std::max<long long>(8, std::min<long long>(h->opt_n_groups > 0 ? 1000 : 256, ((g + 7) / 8) * 8));
    return (int)g;
}

// Tapered shares (kernels.hpp group_start) pay when the launch has many rounds of workgroups; with few rounds the large
// early shares would simply finish last (measured on the translation sweep, profiles/taper_sweep.sh: -3.5 % at 15
// rounds, -4 % at 8, about even at 4, +14 % at 2) ...
void pick_taper(const coreg_handle* h, int n_groups, int n_batches, int* tmin, int* tfrac) {
    *tmin = (int)h->opt_taper_min;
    if (h->opt_taper_frac >= 0) {
        *tfrac = (int)h->opt_taper_frac;
        return;
    }
    // ... and when the groups are many (a fine taper) -- cfg4's 16 groups of a 156-tile grid lost 27 % to it, the
    // 4-round plate-carree launch 20 %
    const double rounds = (double)n_groups * n_batches / 256.0;
    *tfrac = (rounds >= (double)h->opt_taper_rounds && n_groups >= 128 && h->opt_shard_world <= 1) ? 512 : 0;
}

template <int MODE>
int launch_precompute(coreg_handle* h, const PrecomputeArgs& a, int n_tiles, int n_groups, int n_batches) {
    EventPair* ev = next_event(h, h->ev_pre, h->ev_pre_used);
    if (!ev) return fail(h, COREG_EHIP, "hipEventCreate failed");
    int tmin, tfrac;
    pick_taper(h, n_groups, n_batches, &tmin, &tfrac);
    PrecomputeArgs b = a;
    b.prologue = h->pending_prologue;  // (the first launch after upload_plan carries the sweep's prologue)
    const bool with_prologue = b.prologue.src != nullptr;
    std::memset(&h->pending_prologue, 0, sizeof(h->pending_prologue));
    HIPCHK(hipEventRecord(ev->a, h->stream));
    if (h->ref_dtype == COREG_F32)
        hipLaunchKernelGGL((k_precompute<MODE, float>), dim3(n_tiles), dim3(256), 0, h->stream, b);
    else
        hipLaunchKernelGGL((k_precompute<MODE, double>), dim3(n_tiles), dim3(256), 0, h->stream, b);
    (void)with_prologue;
    hipLaunchKernelGGL(k_tile_list, dim3(1), dim3(1024), 0, h->stream, (const int*)a.tile_count, n_tiles, n_groups,
                       h->tile_list.as<int>(), h->tile_cum.as<int>(), h->group_first.as<int>(),
                       h->tile_info.as<long long>(), tmin, tfrac);
    // (no closing event: the sweep launch that follows opens with one, and that is where this interval ends --
    // collect_stats; one marker packet less between the kernels of a sweep)
    ev->b_is_next_sweep = true;
    ev->next_sweep_index = h->ev_sweep_used;
    HIPCHK(hipGetLastError());
    return COREG_OK;
}

int reserve_tiles(coreg_handle* h, int n_tiles) {
    // + an explicit tail: the rolling scalar prefetch of tile_points reads up to kPointGroups chunks past a tile's last
    // chunk (never used), which for the last tile is past the requested size whatever capacity an earlier, larger
    // reservation left
    const size_t pts = (size_t)n_tiles * kTilePts + (size_t)(kPointGroups + 1) * kChunk;
    HIPCHK(h->pts.reserve(pts * sizeof(Pt)));
    HIPCHK(h->tile_count.reserve(n_tiles * sizeof(int)));
    HIPCHK(h->tile_list.reserve(n_tiles * sizeof(int)));
    HIPCHK(h->tile_cum.reserve((n_tiles + 1) * sizeof(int)));
    HIPCHK(h->group_first.reserve(2 * 1024 * sizeof(int) + 64));  // [0, 1024): first list entry; [1024, ...): first unit
    HIPCHK(h->tile_info.reserve(8 * sizeof(long long)));
    HIPCHK(h->tile_bbox.reserve((size_t)n_tiles * 4 * sizeof(double)));
    return COREG_OK;
}

// the precompute arguments every sweep shares (the rest zero), with the tile buffers reserved for the plan's tile shape
int setup_precompute(coreg_handle* h, const Plan& plan, int method, PrecomputeArgs* a, int* n_tiles) {
    std::memset(a, 0, sizeof(*a));
    a->tile_w = plan.tile_w;
    a->tile_h = kTilePts / plan.tile_w;
    a->tiles_x = (h->gW + a->tile_w - 1) / a->tile_w;
    a->tiles_y = (h->gH + a->tile_h - 1) / a->tile_h;
    *n_tiles = a->tiles_x * a->tiles_y;
    RETCHK(reserve_tiles(h, *n_tiles));
    a->ref = h->ref.p;
    a->gw = h->gW;
    a->gh = h->gH;
    a->pivot_a = h->pivots.as<double>();
    a->pts = h->pts.as<Pt>();
    a->tile_count = h->tile_count.as<int>();
    a->tile_bbox = h->tile_bbox.as<double>();
    a->residus = method != COREG_METHOD_CORRELATION ? 1 : 0;  // (both residus methods)
    return COREG_OK;
}

// one sweep-kernel launch + finalize over n_batches * 256 slots whose parameters (SoA [np][n_slots]) and output
// indices are already on the device
long long lds_window_elems(const coreg_handle* h);

// Compile-time LDS window pitch of a launch (lag_plan::pitch_for) under the handle's options.  0 = pitch chosen per visit.
int pick_pitch(const coreg_handle* h, const Plan& plan, long long lds_elems, int order = 2) {
    if (h->opt_pitch == 0 || !h->opt_use_lds) return 0;
    if (h->opt_pitch > 0) {
        for (int p : {89, 121, 153, 185, 217})
            if (p == h->opt_pitch) return p;
        return 0;
    }
    return lag_plan::pitch_for(plan, lds_elems, order);
}

}  // namespace
