"""
k_sweep's walk over the compacted points of a tile (kernels_sweep.hpp tile_points): one running pointer per point-group,
advanced once per chunk of four points, the chunk's four prefetches at immediate offsets from it; in the interior loops
the prefetch has no wait of its own (the gather's wait drains it).  What can go wrong is the walk itself, so the shapes
are the smallest that reach its edges.

Carrington order-2 sweeps of a 64 x 64 image over grids of 49 to 90 points a side laid on the inner window of
tests/sweep_variant_cases.py (every grid point has a finite reference: asserted from last_stats(), so a tile's point
count is the area of its rectangle), points cut in the fewest shares (n_groups 8), under 3 x 3 and 5 x 4 lags:

  grid     tile      tiles' point counts c          n_full = c // 4, n_full % 4, tail c % 4
  64 x 64  32 x 32   1024                           256, 0, 0   every tile full -- the last one too, whose last chunks
                                                                 prefetch past the tile buffer into its padding
  53 x 53  1024 x 1  53                             13, 1, 1
  90 x 90  1024 x 1  90                             22, 2, 2
  63 x 63  1024 x 1  63                             15, 3, 3
  49 x 51  32 x 32   1024, 544, 608, 323            ... and 80, 0, 3 in the corner tile

(n_full % 4 names the point-group that owns the ragged tail; the table is recomputed from the shapes and asserted, not
assumed.)  Each grid runs
  clean     on the all-finite image: every visit interior and all-finite, the loop without the sample mask;
  masked    with 0.5 % NaN pixels: every visit interior, the masked loop;
  bounded   with the NaN image under lags that carry the image's edge across the grid: no visit interior;
each with the device's own residency (sweep_wgs 0) and with one workgroup per queue (sweep_wgs 8).  One helioprojective
order-2 sweep walks the loop that advances along runs (h_incr).

Maps against the CPU oracle at 1e-10 (Carrington) and 1e-7 (helioprojective), per-lag sample counts exactly, and no
lag-point re-evaluated (refined_lag_points == 0): a wrong sweep is not repaired behind the test.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import masked_scores_oracle as M
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import assert_counts

N = 64
PX = 1007.616 / N
CHUNK, POINT_GROUPS, TILE_POINTS = 4, 4, 1024
DEFAULTS = {"n_groups": 0, "tile_w": 0, "sweep_wgs": 0}

# name -> (grid shape, tile_w, {(n_full % 4, tail)} the grid's tiles must show)
GRIDS = {
    "64x64-full-tiles": ((64, 64), 32, {(0, 0)}),
    "53x53-rows": ((53, 53), 1024, {(1, 1)}),
    "90x90-rows": ((90, 90), 1024, {(2, 2)}),
    "63x63-rows": ((63, 63), 1024, {(3, 3)}),
    "49x51-corner": ((49, 51), 32, {(0, 0), (0, 3)}),
}
# interior: whole pixels and half pixels about the pointing error, the inner window stays inside the image;
# bounded: steps of a quarter of the image and more, the image's edge crosses the window
LAGS = {
    ("interior", "3x3"): (17.0 + PX * np.arange(-1, 2), -9.0 + PX * np.arange(-1, 2), None, None, None),
    ("interior", "5x4"): (17.0 + PX * np.arange(-2, 3), -9.0 + PX * np.array([-1.5, -0.5, 0.5, 1.5]), None, None, None),
    ("bounded", "3x3"): (17.0 + PX * np.array([-28.0, 0.0, 28.0]), -9.0 + PX * np.array([-22.0, 0.0, 22.0]), None, None,
                         None),
    ("bounded", "5x4"): (17.0 + PX * np.array([-28.0, -14.0, 0.0, 14.0, 28.0]),
                         -9.0 + PX * np.array([-22.0, -7.5, 7.5, 22.0]), None, None, None),
}


def tile_classes(shape, tile_w):
    """{(n_full % 4, tail)} over the tiles of a grid whose every point is kept, and the last tile's point count."""
    tile_h = TILE_POINTS // tile_w
    out, last = set(), 0
    for y0 in range(0, shape[1], tile_h):
        for x0 in range(0, shape[0], tile_w):
            c = min(tile_w, shape[0] - x0) * min(tile_h, shape[1] - y0)
            out.add(((c // CHUNK) % POINT_GROUPS, c % CHUNK))
            last = c
    return out, last


@functools.lru_cache(maxsize=None)
def images():
    small, hs, large, hl, _ = H.scene(small_n=N, large_n=96, nan_frac=0.0)
    nan = small.copy()
    nan[np.random.default_rng(29).random(nan.shape) < 0.005] = np.nan
    for a in (small, nan, large):
        a.setflags(write=False)
    return {"clean": small, "masked": nan, "bounded": nan}, hs, large, hl


@functools.lru_cache(maxsize=None)
def oracle(grid, kind, lagset):
    """(map, per-lag counts) of the CPU oracle; computed once, never modified."""
    imgs, hs, large, hl = images()
    shape = GRIDS[grid][0]
    lags = LAGS[("bounded" if kind == "bounded" else "interior", lagset)]
    g = dict(shape=shape, lonlims=V.INNER_GRID["lonlims"], latlims=V.INNER_GRID["latlims"])
    want = H.oracle_carrington(imgs[kind], hs, large, hl, lags, **g)
    st = H.oracle_state(imgs[kind], hs, large, hl, lags, shape=list(shape), lonlims=list(g["lonlims"]),
                        latlims=list(g["latlims"]), solar_r=(1.004,))
    m = M.sweep(st, "carrington")
    assert m["poisoned"].sum() == 0 and np.array_equal(m["finite_terms"], m["count"])
    for a in (want, m["count"]):
        a.setflags(write=False)
    return want, m["count"], lags, g


def test_the_grids_cover_every_tail_owner_and_every_tail_length():
    seen = set()
    for name, (shape, tile_w, expect) in GRIDS.items():
        got, last = tile_classes(shape, tile_w)
        assert got == expect, (name, got)
        assert 48 <= min(shape) and max(shape) <= 96, name
        seen |= got
    assert {c[0] for c in seen} == {0, 1, 2, 3} and {c[1] for c in seen} == {0, 1, 2, 3}, seen
    # the grid of full tiles: the last tile of the last group is full, its read-ahead leaves the tile buffer
    assert tile_classes(*GRIDS["64x64-full-tiles"][:2])[1] == TILE_POINTS


@pytest.mark.gpu
@pytest.mark.parametrize("sweep_wgs", [0, 8])
@pytest.mark.parametrize("kind", ["clean", "masked", "bounded"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_point_walk_carrington(gpu_handle, grid, kind, sweep_wgs):
    from euispice_coreg_amd import _lib
    h = gpu_handle
    imgs, hs, large, hl = images()
    shape, tile_w, expect = GRIDS[grid]
    for lagset in ("3x3", "5x4"):
        want, counts, lags, g = oracle(grid, kind, lagset)
        what = f"{grid} {kind} {lagset} sweep_wgs={sweep_wgs}"
        gg = _lib.Grid(g["lonlims"], g["latlims"], g["shape"])
        ls = _lib.LagSet(*lags)
        h.set_small(np.array(imgs[kind]))
        h.prepare_reference_carrington(np.array(large), hl, gg, 1.004, 2)
        try:
            for name, value in dict(n_groups=8, tile_w=tile_w, sweep_wgs=sweep_wgs).items():
                h.set_option(name, value)
            got = h.sweep_carrington(hs, gg, 1.004, ls, order=2).reshape(ls.shape + (1,))
        finally:
            for name, value in DEFAULTS.items():
                h.set_option(name, value)
        n, vc = h.last_counts().reshape(ls.shape + (1,)), h.last_visit_counts()
        st, v = h.last_stats(), h.last_sweep_variant()
        print(f"\n[point walk] {what}: {vc}, kernel {v}, points {st['n_active_points']} of {st['n_grid_points']}, "
              f"max|dcorr| = {np.nanmax(np.abs(got - want)) if np.isfinite(want).any() else float('nan'):.3e}")
        # every grid point is kept, so the tiles' point counts are the areas tile_classes() works from
        assert st["n_grid_points"] == st["n_active_points"] == shape[0] * shape[1], st
        assert tile_classes(shape, tile_w)[0] == expect
        assert (v["mode"], v["order"], v["resid"]) == (V.TRANSLATE, 2, False), v
        assert st["used_lds"] == 1 and vc["lds"] == vc["visits"] > 0, vc
        if kind == "clean":
            assert vc["all_finite"] == vc["interior"] == vc["visits"], vc
        elif kind == "masked":
            assert vc["all_finite"] < vc["interior"] == vc["visits"], vc
        else:
            assert vc["interior"] == 0, vc
            assert np.nanmin(counts) < np.nanmax(counts) <= shape[0] * shape[1] and np.nanmax(counts) > 0  # (the rule cuts)
        assert vc["refined_lag_points"] == 0, vc
        assert_counts(n, counts, what)
        H.assert_corr_close(got, want, 1e-10, what)


@pytest.mark.gpu
def test_point_walk_along_runs_helioprojective(gpu_handle):
    """Order 2 on the helioprojective frame: interior LDS visits of the homography advance along runs of a grid row
    (tile_points, kIncr), the third of the loops that share the running pointer."""
    h = gpu_handle
    sc = V.scene("helio-series", True, "interior")
    small, hs, large, hl, lags = sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"]
    want = H.oracle_helio(small, hs, large, hl, lags, order=2)
    m = M.sweep(H.oracle_state(small, hs, large, hl, lags, order=2), "helioprojective")
    assert m["poisoned"].sum() == 0
    for sweep_wgs in (0, 8):
        try:
            h.set_option("sweep_wgs", sweep_wgs)
            got = H.gpu_helio(h, small, hs, large, hl, lags, order=2)
        finally:
            h.set_option("sweep_wgs", 0)
        v, vc = h.last_sweep_variant(), h.last_visit_counts()
        print(f"\n[point walk] helioprojective sweep_wgs={sweep_wgs}: {vc}, kernel {v}, "
              f"max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
        assert v["mode"] in (V.HOMOGRAPHY, V.HOMOGRAPHY_SERIES) and v["order"] == 2 and not v["resid"], v
        assert vc["interior"] > 0 and vc["refined_lag_points"] == 0, vc
        assert_counts(h.last_counts(), m["finite_terms"], f"helioprojective sweep_wgs={sweep_wgs}")
        H.assert_corr_close(got, want, 1e-7, f"helioprojective sweep_wgs={sweep_wgs}")
