// Part of libcoreg_hip.so's ONE translation unit (coreg_hip.hip includes the parts in order; round 6 split by concern,
// no behaviour change): what a sweep needs of the handle before its launches: lag dimensions and checks, tile groups, tapered shares, the precompute launch and its buffers.
#pragma once
namespace {
// (sweep_plan.hpp, plain C++: parallel_for, the lag planner under the handle's options, the pure rules pick_groups /
// pick_pitch, and the three planners of the header-shift sweeps)

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

// tile groups of a launch under the handle's options (sweep_plan.hpp pick_groups)
int pick_groups(const coreg_handle* h, int n_batches, int n_tiles) {
    (void)n_tiles;
    return coreg::pick_groups(h->opt_shard_world, h->opt_n_groups, n_batches);
}

// What the planners of the header-shift sweeps (sweep_plan.hpp) may read of the handle, and the state they may update:
// the wcslib caches and the lag-plan memo.
long long lds_window_elems(const coreg_handle* h);
SweepEnv sweep_env(coreg_handle* h) {
    SweepEnv e;
    e.sW = h->sW;
    e.sH = h->sH;
    e.gW = h->gW;
    e.gH = h->gH;
    e.border_fix = h->opt_border_fix != 0;
    e.tap_fix = h->opt_tap_fix != 0;
    e.use_lds = h->opt_use_lds != 0;
    e.h_series = h->opt_h_series != 0;
    e.tile_skip = h->opt_tile_skip != 0;
    e.lds_elems = lds_window_elems(h);
    e.tile_w = (int)h->opt_tile_w;
    e.patch_w = (int)h->opt_patch_w;
    e.shard_world = h->opt_shard_world;
    e.n_groups = h->opt_n_groups;
    e.pitch = h->opt_pitch;
    e.tabs = &h->tabs;
    e.caches = &h->wcslib;
    e.memo = &h->plan_memo;
    return e;
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
                       h->tile_info.as<long long>(), tmin, tfrac, (const double*)a.tile_bbox,
                       h->visit_rec.as<VisitRec>());
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
    HIPCHK(h->visit_rec.reserve(((size_t)n_tiles + 1) * sizeof(VisitRec)));  // one per list entry + the sentinel
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

}  // namespace
