"""
What opens a tile visit of k_sweep (kernels_sweep.hpp): the visit record of the tile-list entry (k_tile_list's VisitRec,
read one visit ahead through the scalar path and parked in a VGPR), for the translation the box of the visit from the
lag extents reduced once per launch, and the one-fma staging of the order-2 window.  None of it may change a sample, a
sum or a visit decision, so every case is held to the CPU oracles at the project's bounds -- 1e-10 where every visit is
interior, 1e-9 on the Carrington frame otherwise, 1e-7 on the helioprojective frame -- and its tile-visit counters
(coreg_last_visit_counts: all, LDS-staged, interior, all-finite interior) to those of the commit before the change.

PARENT_COUNTS were read on that commit (d7400ac) by running this file's cases on its library on an MI355X and copying the
`[visit setup] key: counts` lines it prints; the map of every case was within the same bounds there.

Scenes: tests/test_gpu_scalar_count.py's, H.scene(small_n=96, large_n=96) and the 24^2 image of its bounded cases.

  1. interior         grid 64 x 64 on the inner window, tile_w 64 (4 tiles of 64 x 16 points), n_groups 8: every other
                      group's share begins inside a tile.  taper_frac 0 and the default; orders 1, 2, 3; float32-exact
                      and float64 pixels; the generic and the pitched kernel.  5 x 5 lags: three of the four lag-waves
                      are padding (NaN lanes the lag extents must ignore).
     many visits      the same window sampled 256 x 256 (64 tiles): a workgroup of the 8 walks 8 or 9 list entries, so
                      the record read ahead is used visit after visit (order 2, both kernels).
  2. two batches      18 x 18 lags on the 40 x 36 grid that is wider than the image's field of view: tiles are live
                      under one batch and culled under the other, and the last list entry is live (the sentinel record
                      after it ends the walk).
  3. ragged patch     17 x 15 lags: 255 slots, the last lag-wave one lane short.
  4. image 24^2       no interior visit; also with use_lds 0 and with the smallest lds_bytes.  The library's floor on the
                      window (36 KiB, its closing reduction) holds any window of a 24^2 image, so the visits that fall
                      back to the global-memory gather beside staged ones are those of case 2's 96^2 sweep under the
                      same lds_bytes.
  5. series homography on the helioprojective frame: reads the records, keeps the per-visit box reduction.
  6. point shard      set_point_shard(1, 2): the launch's first group is not group 0.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import CARR_RTOL
from tests.test_gpu_scalar_count import B_GRID, B_LAGS, GRID, LAGS, N, PX, bounded_scene

pytestmark = pytest.mark.gpu

assert CARR_RTOL == 1e-10
OPTION_DEFAULTS = {"pitch": -1, "n_groups": 0, "tile_w": 0, "taper_frac": -1, "use_lds": 1,
                   "lds_bytes": (159 * 1024 * 4) // 4}
KINDS = ("visits", "lds", "interior", "all_finite")

# key -> (visits, lds, interior, all_finite) on the parent commit (see the module docstring)
PARENT_COUNTS = {
    "interior o1 f32 generic taper 0": (8, 8, 8, 8),
    "interior o1 f32 generic taper -1": (8, 8, 8, 8),
    "interior o1 f32 pitched taper 0": (8, 8, 8, 8),
    "interior o1 f32 pitched taper -1": (8, 8, 8, 8),
    "interior o1 f64 generic taper 0": (8, 8, 8, 8),
    "interior o1 f64 generic taper -1": (8, 8, 8, 8),
    "interior o1 f64 pitched taper 0": (8, 8, 8, 8),
    "interior o1 f64 pitched taper -1": (8, 8, 8, 8),
    "interior o2 f32 generic taper 0": (8, 8, 8, 8),
    "interior o2 f32 generic taper -1": (8, 8, 8, 8),
    "interior o2 f32 pitched taper 0": (8, 8, 8, 8),
    "interior o2 f32 pitched taper -1": (8, 8, 8, 8),
    "interior o2 f64 generic taper 0": (8, 8, 8, 8),
    "interior o2 f64 generic taper -1": (8, 8, 8, 8),
    "interior o2 f64 pitched taper 0": (8, 8, 8, 8),
    "interior o2 f64 pitched taper -1": (8, 8, 8, 8),
    "interior o3 f32 generic taper 0": (8, 8, 8, 8),
    "interior o3 f32 generic taper -1": (8, 8, 8, 8),
    "interior o3 f32 pitched taper 0": (8, 8, 8, 8),
    "interior o3 f32 pitched taper -1": (8, 8, 8, 8),
    "interior o3 f64 generic taper 0": (8, 8, 8, 8),
    "interior o3 f64 generic taper -1": (8, 8, 8, 8),
    "interior o3 f64 pitched taper 0": (8, 8, 8, 8),
    "interior o3 f64 pitched taper -1": (8, 8, 8, 8),
    "many visits generic": (64, 64, 64, 64),
    "many visits pitched": (64, 64, 64, 64),
    "two batches generic": (213, 213, 0, 0),
    "two batches pitched": (213, 213, 0, 0),
    "ragged 17x15 generic": (8, 8, 8, 8),
    "ragged 17x15 pitched": (8, 8, 8, 8),
    "24^2 lds generic": (90, 90, 0, 0),
    "24^2 lds pitched": (90, 90, 0, 0),
    "24^2 no lds generic": (90, 0, 0, 0),
    "24^2 no lds pitched": (90, 0, 0, 0),
    "24^2 small lds generic": (162, 162, 0, 0),
    "24^2 small lds pitched": (162, 162, 0, 0),
    "96^2 small lds generic": (213, 13, 0, 0),
    "96^2 small lds pitched": (213, 13, 0, 0),
    "helio series generic": (522, 522, 116, 116),
    "helio series pitched": (522, 522, 116, 116),
    "point share 0 of 2": (128, 128, 128, 128),
    "point share 1 of 2": (128, 128, 128, 128),
}


def counts(vc):
    return tuple(int(vc[k]) for k in KINDS)


class Ledger:
    """Collects (key, counters) of a test's sweeps; `settle` prints them all, then holds them to PARENT_COUNTS."""

    def __init__(self):
        self.seen = []

    def add(self, key, vc):
        print(f"\n[visit setup] {key!r}: {counts(vc)},")
        self.seen.append((key, counts(vc)))

    def settle(self):
        wrong = [(k, c, PARENT_COUNTS.get(k)) for k, c in self.seen if PARENT_COUNTS.get(k) != c]
        assert not wrong, f"tile-visit counters differ from the parent commit's (key, got, parent): {wrong}"


@functools.lru_cache(maxsize=None)
def scene96(f32_exact):
    small, hs, large, hl, _ = H.scene(small_n=N, large_n=N, nan_frac=0.0, float32_exact=f32_exact)
    for a in (small, large):
        a.setflags(write=False)
    return small, hs, large, hl


def carrington(h, small, hs, large, hl, lags, grid, order, **options):
    """One sweep under `options` (restored afterwards): (6-D map, visit counters, kernel that ran)."""
    from euispice_coreg_amd import _lib
    g = _lib.Grid(grid["lonlims"], grid["latlims"], grid["shape"])
    ls = _lib.LagSet(*lags)
    h.set_small(np.array(small))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, order)
    try:
        for name, value in options.items():
            h.set_option(name, value)
        out = h.sweep_carrington(hs, g, 1.004, ls, order=order)
    finally:
        for name, value in OPTION_DEFAULTS.items():
            h.set_option(name, value)
    return out.reshape(ls.shape + (1,)), h.last_visit_counts(), h.last_sweep_variant()


def bound(vc):
    """The project's bound on the Carrington frame: 1e-10 when every visit ran the interior loop, else 1e-9."""
    return 1e-10 if vc["interior"] == vc["visits"] else 1e-9


def check(got, want, vc, what, atol=None):
    atol = bound(vc) if atol is None else atol
    print(f"[visit setup] {what}: max|dcorr| = {np.nanmax(np.abs(got - want)):.3e} (bound {atol:.0e})")
    H.assert_corr_close(got, want, atol, what)


PITCHES = ((0, "generic"), (-1, "pitched"))


# ---- 1. interior ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32_exact", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_interior_shares_that_begin_inside_a_tile(gpu_handle, order, f32_exact):
    small, hs, large, hl = scene96(f32_exact)
    want = H.oracle_carrington(small, hs, large, hl, LAGS, order=order, **GRID)
    led = Ledger()
    for pitch, pname in PITCHES:
        for taper in (0, -1):
            key = f"interior o{order} {'f32' if f32_exact else 'f64'} {pname} taper {taper}"
            got, vc, v = carrington(gpu_handle, small, hs, large, hl, LAGS, GRID, order, pitch=pitch, n_groups=8,
                                    tile_w=64, taper_frac=taper)
            led.add(key, vc)
            assert (v["mode"], v["order"], v["f32"]) == (V.TRANSLATE, order, int(f32_exact)), v
            # (orders 1 and 3 have no pitched instantiation for every pixel type: the pick is the library's)
            assert vc["interior"] == vc["lds"] == vc["visits"] >= 8, vc  # 8 groups, each at least one visit, all interior
            check(got, want, vc, key, 1e-10)
    led.settle()


def test_interior_many_visits_per_workgroup(gpu_handle):
    small, hs, large, hl = scene96(True)
    grid = dict(GRID, shape=(256, 256))
    want = H.oracle_carrington(small, hs, large, hl, LAGS, order=2, **grid)
    led = Ledger()
    for pitch, pname in PITCHES:
        key = f"many visits {pname}"
        got, vc, _ = carrington(gpu_handle, small, hs, large, hl, LAGS, grid, 2, pitch=pitch, n_groups=8, tile_w=64,
                                taper_frac=0)
        led.add(key, vc)
        assert vc["interior"] == vc["visits"] >= 64, vc  # 64 tiles cut in 8 shares: 8 entries a workgroup, or 9
        check(got, want, vc, key, 1e-10)
    led.settle()


# ---- 2., 3. lag planes of more than one batch, and of a ragged last wave ----------------------------------------------
def plane(n1, n2):
    return (17.0 + PX * (np.arange(n1) - n1 // 2), -9.0 + PX * (np.arange(n2) - n2 // 2), None, None, None)


def test_two_batches_on_a_grid_wider_than_the_field_of_view(gpu_handle):
    small, hs, large, hl = scene96(True)
    lags = plane(18, 18)
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **V.BORDER_GRID)
    led = Ledger()
    for pitch, pname in PITCHES:
        key = f"two batches {pname}"
        got, vc, _ = carrington(gpu_handle, small, hs, large, hl, lags, V.BORDER_GRID, 2, pitch=pitch)
        led.add(key, vc)
        assert vc["interior"] < vc["visits"], vc  # (the grid leaves the image: visits under the bounds rule)
        check(got, want, vc, key, 1e-9)
    led.settle()


def test_ragged_last_lag_wave(gpu_handle):
    small, hs, large, hl = scene96(True)
    lags = plane(17, 15)
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **GRID)
    led = Ledger()
    for pitch, pname in PITCHES:
        key = f"ragged 17x15 {pname}"
        got, vc, _ = carrington(gpu_handle, small, hs, large, hl, lags, GRID, 2, pitch=pitch, n_groups=8, tile_w=64)
        led.add(key, vc)
        check(got, want, vc, key)
    led.settle()


# ---- 4. image 24^2: no interior visit ---------------------------------------------------------------------------------
SMALL_LDS_BYTES = 1024  # the smallest the option takes


def test_bounded_visits_lds_global_and_mixed(gpu_handle):
    small, hs, large, hl = bounded_scene()
    want = H.oracle_carrington(small, hs, large, hl, B_LAGS, order=2, **B_GRID)
    led = Ledger()
    for name, options in (("lds", {}), ("no lds", {"use_lds": 0}), ("small lds", {"lds_bytes": SMALL_LDS_BYTES})):
        for pitch, pname in PITCHES:
            key = f"24^2 {name} {pname}"
            got, vc, _ = carrington(gpu_handle, small, hs, large, hl, B_LAGS, B_GRID, 2, pitch=pitch, **options)
            led.add(key, vc)
            assert vc["interior"] == 0 < vc["visits"], vc
            # (the library never takes less LDS than the 36 KiB its closing reduction needs, and that holds the whole
            # 24^2 image with its apron: "small lds" changes the plan here, the mix of paths is the 96^2 case below)
            assert vc["lds"] == (0 if name == "no lds" else vc["visits"]), vc
            check(got, want, vc, key, 1e-9)
    # the 96^2 image under the smallest window: most visits of the two-batch case gather from global memory, some stage
    small, hs, large, hl = scene96(True)
    lags = plane(18, 18)
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **V.BORDER_GRID)
    for pitch, pname in PITCHES:
        key = f"96^2 small lds {pname}"
        got, vc, _ = carrington(gpu_handle, small, hs, large, hl, lags, V.BORDER_GRID, 2, pitch=pitch,
                                lds_bytes=SMALL_LDS_BYTES)
        led.add(key, vc)
        assert 0 < vc["lds"] < vc["visits"], vc
        check(got, want, vc, key, 1e-9)
    led.settle()


# ---- 5. the series homography -----------------------------------------------------------------------------------------
def test_series_homography_reads_the_records(gpu_handle):
    sc = V.scene("helio-series", True, "interior")
    small, hs, large, hl, lags = sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"]
    want = H.oracle_helio(small, hs, large, hl, lags, order=2)
    h = gpu_handle
    led = Ledger()
    for pitch, pname in PITCHES:
        try:
            h.set_option("pitch", pitch)
            got = H.gpu_helio(h, small, hs, large, hl, lags, order=2)
        finally:
            h.set_option("pitch", -1)
        v, vc = h.last_sweep_variant(), h.last_visit_counts()
        key = f"helio series {pname}"
        led.add(key, vc)
        assert (v["mode"], v["order"]) == (V.HOMOGRAPHY_SERIES, 2), v
        assert 0 < vc["interior"] < vc["lds"], vc  # the middle tile of the 3 x 3 is interior, the outer ones are not
        check(got, want, vc, key, 1e-7)
    led.settle()


# ---- 6. a launch whose first group is not group 0 ---------------------------------------------------------------------
def test_second_point_share(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl = scene96(True)
    want = H.oracle_carrington(small, hs, large, hl, LAGS, order=2, **GRID)
    h = gpu_handle
    g = _lib.Grid(GRID["lonlims"], GRID["latlims"], GRID["shape"])
    ls = _lib.LagSet(*LAGS)
    h.set_small(np.array(small))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, 2)
    led = Ledger()
    try:
        h.set_option("tile_w", 64)
        total = None
        for r in range(2):
            h.set_point_shard(r, 2)
            assert np.isnan(h.sweep_carrington(hs, g, 1.004, ls)).all()
            led.add(f"point share {r} of 2", h.last_visit_counts())
            s = h.copy_sums()
            total = s if total is None else total + s
        got = h.finalize_sums(total, ls.size).reshape(ls.shape + (1,))
    finally:
        h.set_point_shard(0, 1)
        h.set_option("tile_w", 0)
    check(got, want, dict(interior=1, visits=1), "two point shares, added", 1e-10)
    led.settle()
