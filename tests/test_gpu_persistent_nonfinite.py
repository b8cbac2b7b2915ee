"""
k_sweep's persistent workgroups on images with NaN and infinite pixels (kernels_sweep.hpp).  The workgroup state that
outlives a tile visit, and since the persistent loop an item -- wdirty[visit & 1][wave] ("this wave staged a NaN or an
infinity": it picks the CLEAN variant of tile_points, which drops the per-sample finite mask), the visit parity that
restarts with every item while the LDS slots do not, wred2 (the item's lag extents on the translate path, the per-visit
boxes on the homography path) and the reduction scratch that aliases the staged window -- only matters when dirty and
clean windows meet in one item, and in the items one workgroup runs one after another.  tests/test_gpu_visit_setup.py and
tests/test_gpu_persistent_sweep.py have no non-finite pixel; tests/test_gpu_scalar_count.py has one visit per item and one
item per workgroup.

Every sweep here runs through `three_ways_counts`: three_ways of tests/test_gpu_persistent_sweep.py (the map against the
CPU oracle under one item per workgroup; bitwise the same map and the same four visit counters under sweep_wgs 8, 12
and 0) and, on top, the per-lag sample counts (last_counts) of every one of those sweeps: equal to the oracle's
`finite_terms` exactly and bitwise the same under every cap.  The counts are integers that differ from lag to lag once
pixels are masked, so an unmasked sample, a sample masked twice or a lost visit shows in them whatever the map's bound.

1. Carrington frame (translate path), mixed visits.  The 96^2 scene; a 256 x 256 grid over lon 237-253, lat -1-11 with
   tile_w 64, n_groups 8, taper_frac 0: 64 tiles of 64 x 16 points in 4 tile columns x 16 tile rows, tiles in row-major
   order (k_precompute: tile = ty * tiles_x + tx; k_tile_list keeps that order), 8 tiles an item, so an item visits the
   tile columns 0, 1, 2, 3, 0, ... and ends on column 3; 17 x 17 lags an eighth of a pixel apart (two batches, the second
   ragged).  Every visit is interior (asserted), so every visit reaches the clean-path decision.

   Images: the finite image with whole pixel columns set to NaN (in image P one of them to +inf: staging detects
   non-finite values through 0 * e, and an infinity takes that route by another door).  Column X[c] lies under tile column
   c alone:

   PRECONDITION (asserted on the CPU, from the oracle's sample coordinates O.carrington_coords at the four corner lags of
   the plane, for every one of the 64 tiles).  With lo_l, hi_l the x-box of the tile's samples under corner lag l and
   (ap_lo, ap_hi) the apron of the spline order (kernels_sweep.hpp: 1, 2 for orders 1 and 2; 2, 3 for order 3), the
   kernel's window is [floor(mnx) - ap_lo, floor(mxx) + ap_hi] with mnx, mxx the box over the item's lags -- any subset
   of the plane.  A pixel column x is CERTAINLY STAGED by the tile when
       floor(max_l lo_l) - ap_lo + 1 <= x <= floor(min_l hi_l) + ap_hi - 1
   (the window of any subset, shrunk by one pixel) and CERTAINLY NOT STAGED when it lies outside
       [floor(min_l lo_l) - ap_lo - 1, floor(max_l hi_l) + ap_hi + 1]
   (the largest window, grown by one pixel).  X[c] is certainly staged by the 16 tiles of column c and certainly not
   staged by the other 48, at orders 1, 2 and 3.  (A grid over lon 240-252 leaves tile column 1 two such pixels at
   order 2 and none at order 3; this one leaves every column at least four at every order.)

   Four images in two complementary pairs (dirty tile columns):
     P {0, 2} / P' {1, 3}   visits alternate dirty, clean: each parity slot of wdirty holds one value for the whole item,
                            the two slots different ones -- a flag read from the other slot is wrong at every visit.
     Q {0, 1} / Q' {2, 3}   dirty, dirty, clean, clean: each parity slot alternates, so a slot that kept its previous
                            content (a write that is skipped, or read before it lands) is wrong at every second visit;
                            an item ends clean and the workgroup's next one starts dirty in Q, the other way in Q'.
   (A library that merely uses ONE slot for both parities, written and read through the same pointer, is not wrong: a
   live visit has two barriers between its write and the next write of any slot.  It passes this module, as it must.
   One that reads slot 0 whatever the parity fails pair P; one that skips the write on clean windows, over slots zeroed
   at kernel entry, fails pair Q and the homography case -- and neither fails anything else in the suite.)

   THE CHECK ON THE FLAG ITSELF does not compare the kernel with itself: the counters visits, lds, interior depend on
   the geometry only (asserted equal for the finite image, X and X'), a visit is all-finite in exactly one image of a
   complementary pair, so all_finite(X) + all_finite(X') == interior with 0 < all_finite(X) < interior.  A stale dirty
   flag makes the sum too small (and costs only speed: nothing else would show it); a stale clean flag makes it too
   large and puts NaN into the map and wrong numbers into the counts.

   Further on image P: clean_path 0 (all_finite == 0, same map and counts), orders 1 and 3 (clean-path instantiations of
   their own).
2. Methods without a clean path on image Q: plain residus (all NaN, as numpy gives it; counts exact; all_finite 0) and
   the masked residus on a reference with a block <= 0, whose terms are poisoned (asserted on the oracle).
3. Homography path (per-visit wred2 and wdirty, no lag-extent barrier): V.scene("helio-series", True, "interior"),
   13 x 12 x 2 lags (312: two batches) within half a pixel of the pointing error, tile_w 32 (3 x 3 tiles), n_groups 16.
   The oracle's coordinates (O.extract_coordinates_pixels per lag) show tiles (ty, tx) = (0, 1), (0, 2), (1, 1), (1, 2)
   inside the image under every lag and the other five outside under every lag, each by at least 0.01 pixel
   (asserted; the kernel's clearance is 1e-9 and the series homography's coordinates are far closer to the oracle's than
   that margin).  NaN column 45 is certainly staged by the interior tiles of column 1 and certainly not by those of
   column 2, column 80 the other way round (the same rule as above): the same all_finite identity holds and is asserted.
4. Bounded visits under the queues: V.BORDER_GRID, the 96^2 scene with 1 % NaN pixels (fixed seed), the two lag clusters
   of test_items_whose_every_visit_is_culled, n_groups 24.

Bounds (none new): maps 1e-10 (CARR_RTOL) where every visit is interior -- the bound tests/test_gpu_scalar_count.py
holds the masked interior loop to; coefficients are <= 1 in size --, the Carrington frame's rule of three_ways (1e-9)
on the bounded case, 1e-7 on the helioprojective frame, 1e-10 of max|want| for the residus methods (assert_masked);
counts: equality.  tests/test_persistent_nonfinite_cpu.py asserts the preconditions and the oracle's expectations
without a GPU; here the same cached functions run before the first GPU call of each test.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import masked_scores_oracle as M
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import CARR_RTOL, assert_counts, assert_masked
from tests.test_gpu_persistent_sweep import (CAPS, ONE_ITEM_EACH, bitwise, carrington_run, counts, plane, scene96,
                                             three_ways, with_options)
from tests.test_gpu_scalar_count import PX

pytestmark = pytest.mark.gpu

W = 96                                                                  # the image to align is 96 x 96 pixels
GRID = dict(shape=(256, 256), lonlims=(237.0, 253.0), latlims=(-1.0, 11.0))
LAGS = plane(17, 17, 0.125 * PX)                                        # 289 lags: two batches, the second ragged
OPTIONS = dict(n_groups=8, tile_w=64, taper_frac=0)
TILE_W, TILE_H = 64, 16
APRON = {1: (1, 2), 2: (1, 2), 3: (2, 3)}                               # order -> (ap_lo, ap_hi), kernels_sweep.hpp
X = (28, 47, 65, 84)                                                    # X[c]: the pixel column under tile column c alone
# image -> {pixel column: value}
IMAGES = {
    "finite": {},
    "P": {X[0]: np.nan, X[2]: np.inf},
    "P'": {X[1]: np.nan, X[3]: np.nan},
    "Q": {X[0]: np.nan, X[1]: np.nan},
    "Q'": {X[2]: np.nan, X[3]: np.nan},
}
DIRTY = {"finite": (), "P": (0, 2), "P'": (1, 3), "Q": (0, 1), "Q'": (2, 3)}
PAIRS = {"P": ("P", "P'"), "Q": ("Q", "Q'")}


# ---- windows: what a tile certainly stages, what it can stage at most ----------------------------------------------------
def windows(lo, hi, apron):
    """lo, hi: [lag, ...] x-boxes of tiles under some lags.  (certain lo, certain hi, possible lo, possible hi), each
    [...]: the window every subset of those lags stages shrunk by a pixel, the largest one grown by a pixel."""
    ap_lo, ap_hi = apron
    return (np.floor(lo.max(0)) - ap_lo + 1, np.floor(hi.min(0)) + ap_hi - 1,
            np.floor(lo.min(0)) - ap_lo - 1, np.floor(hi.max(0)) + ap_hi + 1)


def certainly_staged(x, win):
    return (win[0] <= x) & (x <= win[1])


def certainly_not_staged(x, win):
    return (x < win[2]) | (x > win[3])


@functools.lru_cache(maxsize=None)
def carrington_boxes():
    """x- and y-boxes [corner lag, tile row, tile column] of the 64 tiles under the four corner lags of LAGS."""
    from oracle import coreg_oracle as O
    small, hs, large, hl = scene96(True)
    st = H.oracle_state(small, hs, large, hl, LAGS, shape=list(GRID["shape"]), lonlims=list(GRID["lonlims"]),
                        latlims=list(GRID["latlims"]), solar_r=(1.004,))
    O.set_initial_header_values(st)
    out = [[], [], [], []]
    for l1 in (LAGS[0][0], LAGS[0][-1]):
        for l2 in (LAGS[1][0], LAGS[1][-1]):
            hdr = dict(st.hdr_small)
            O.shift_header(st, hdr, l1, l2, 0.0, 0.0, 0.0)
            nx, ny = O.carrington_coords(hdr, 1.004, list(GRID["shape"]), list(GRID["lonlims"]), list(GRID["latlims"]))
            assert nx.shape == (256, 256) and np.isfinite(nx).all() and np.isfinite(ny).all()
            for k, t in enumerate((nx, ny)):  # [grid row, grid column] -> [tile row, row in tile, tile column, column in tile]
                t = t.reshape(256 // TILE_H, TILE_H, 256 // TILE_W, TILE_W)
                out[2 * k].append(t.min(axis=(1, 3)))
                out[2 * k + 1].append(t.max(axis=(1, 3)))
    return tuple(np.stack(a) for a in out)


@functools.lru_cache(maxsize=None)
def carrington_precondition(order):
    """Asserts the module docstring's precondition for the spline order; returns the pixel range of the samples."""
    xlo, xhi, ylo, yhi = carrington_boxes()
    # every sample of every lag inside the image, a pixel clear of its edge (the kernel asks for 1e-9): all visits interior
    assert xlo.min() >= 1.0 and xhi.max() <= W - 2.0 and ylo.min() >= 1.0 and yhi.max() <= W - 2.0
    win = windows(xlo, xhi, APRON[order])  # [tile row, tile column]
    for c, x in enumerate(X):
        for t in range(4):
            if t == c:
                assert certainly_staged(x, win)[:, t].all(), (order, c, x, win[0][:, t], win[1][:, t])
            else:
                assert certainly_not_staged(x, win)[:, t].all(), (order, c, x, t, win[2][:, t], win[3][:, t])
    for name, cols in IMAGES.items():  # the images are what DIRTY says
        assert {X.index(x) for x in cols} == set(DIRTY[name]), name
    for a, b in PAIRS.values():
        assert sorted(DIRTY[a] + DIRTY[b]) == [0, 1, 2, 3]
    return xlo.min(), xhi.max(), ylo.min(), yhi.max()


# ---- images and oracles, computed once, never modified -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image(name, f32_exact):
    img = np.array(scene96(f32_exact)[0])
    for x, value in IMAGES[name].items():
        img[:, x] = value
    img.setflags(write=False)
    return img


def _state(img, f32_exact, order, large=None):
    _, hs, ref, hl = scene96(f32_exact)
    return H.oracle_state(img, hs, ref if large is None else large, hl, LAGS, order=order, shape=list(GRID["shape"]),
                          lonlims=list(GRID["lonlims"]), latlims=list(GRID["latlims"]), solar_r=(1.004,))


@functools.lru_cache(maxsize=None)
def oracle_counts(name, f32_exact, order=2):
    """The oracle's per-lag counts of a Carrington image, with what the tests expect of them asserted."""
    carrington_precondition(order)
    m = M.sweep(_state(image(name, f32_exact), f32_exact, order), "carrington")
    n = m["finite_terms"]
    assert m["poisoned"].sum() == 0 and np.array_equal(n, m["count"])
    assert np.isfinite(m["masked"]).all()
    # two pixel columns of ~74 lose their samples: between 5 % and 15 % of the 65 536, and not the same number at every lag
    assert 0.85 * 65536 < n.min() < n.max() < 0.95 * 65536, (name, n.min(), n.max())
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def oracle_map(name, f32_exact, order=2):
    _, hs, large, hl = scene96(f32_exact)
    want = H.oracle_carrington(image(name, f32_exact), hs, large, hl, LAGS, order=order, **GRID)
    assert np.isfinite(want).all()
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def oracle_plain_residus(name, f32_exact):
    from oracle import coreg_oracle as O
    want = O.find_best_header_parameters(_state(image(name, f32_exact), f32_exact, 2), "carrington", method="residus")
    assert np.isnan(want).all()  # (numpy's std over a NaN term: the reference's residus has no number on such an image)
    return want


@functools.lru_cache(maxsize=None)
def poisoned_case(name, f32_exact):
    """(reference with a block <= 0 under the grid, the oracle's masked sweep on it)."""
    from oracle import coreg_oracle as O
    _, _, large, hl = scene96(f32_exact)
    hdr = dict(hl)
    O.check_and_create_pcij_matrix(hdr)
    nx, ny = O.carrington_coords(hdr, 1.004, list(GRID["shape"]), list(GRID["lonlims"]), list(GRID["latlims"]))
    cx, cy = int(np.rint(np.nanmedian(nx))), int(np.rint(np.nanmedian(ny)))
    assert 1 <= cx < large.shape[1] - 2 and 1 <= cy < large.shape[0] - 2, (cx, cy)
    ref = np.array(large)
    ref[cy, cx] = 0.0
    ref[cy, cx + 1] = ref[cy + 1, cx] = ref[cy + 1, cx + 1] = -100.0
    ref.setflags(write=False)
    m = M.sweep(_state(image(name, f32_exact), f32_exact, 2, large=ref), "carrington")
    assert m["poisoned"].sum() > 0 and (m["finite_terms"] == m["count"] - m["poisoned"]).all()
    assert m["finite_terms"].min() > 0 and m["finite_terms"].min() < m["finite_terms"].max()
    return ref, m


# ---- the sweeps ----------------------------------------------------------------------------------------------------------
def three_ways_counts(h, run, want, want_n, atol, what, options, caps=CAPS, close=H.assert_corr_close):
    """three_ways, and the per-lag sample counts of every one of its sweeps: equal to `want_n` exactly, bitwise the same
    under every cap.  Returns (map, visit counters, counts) of the sweep with one item per workgroup."""
    seen = []

    def run_and_keep():
        out = run()
        seen.append(np.array(h.last_counts(), dtype=np.float64).ravel())
        return out

    base, base_counts = three_ways(h, run_and_keep, want, atol, what, options, caps=caps, close=close)
    names = (ONE_ITEM_EACH,) + tuple(caps) + (0,)
    assert len(seen) == len(names), (len(seen), names)
    fin = seen[0][np.isfinite(seen[0])]
    assert fin.size, f"{what}: no lag has a count"
    print(f"[persistent] {what}: counts {fin.min():.0f} ... {fin.max():.0f} over {fin.size} lags, "
          f"equal to the oracle's {np.array_equal(seen[0], np.asarray(want_n, dtype=np.float64).ravel(), equal_nan=True)}")
    for cap, n in zip(names, seen):
        assert_counts(n, want_n, f"{what} sweep_wgs={cap}")
        assert bitwise(n, seen[0]), f"{what}: sweep_wgs={cap} changed the counts"
    return base, base_counts, seen[0]


def under(h, run, **options):
    """`run` under options that with_options does not restore (pitch, clean_path)."""
    def go():
        try:
            for name, value in options.items():
                h.set_option(name, value)
            return run()
        finally:
            h.set_option("pitch", -1)
            h.set_option("clean_path", 1)
    return go


def variant_has_clean_path(h):
    v = h.last_sweep_variant()
    return V.has_clean_path((v["mode"], v["order"], bool(v["f32"]), bool(v["round"]), bool(v["resid"]), v["pitch"]))


def carrington(h, name, f32_exact, pitch, order=2, method=0, clean_path=1, caps=CAPS, want=None, want_n=None,
               close=H.assert_corr_close, large=None, what=None):
    """One image through three_ways_counts; the oracles first.  Returns (visit counters, kernel has a clean path)."""
    want = oracle_map(name, f32_exact, order) if want is None else want
    want_n = oracle_counts(name, f32_exact, order) if want_n is None else want_n
    _, hs, ref, hl = scene96(f32_exact)
    run = under(h, carrington_run(h, image(name, f32_exact), hs, ref if large is None else large, hl, LAGS, GRID, order,
                                  method), pitch=pitch, clean_path=clean_path)
    what = what or f"{name} o{order} {'f32' if f32_exact else 'f64'} pitch {pitch} clean_path {clean_path}"
    _, c, _ = three_ways_counts(h, run, want, want_n, CARR_RTOL, what, OPTIONS, caps=caps, close=close)
    v = h.last_sweep_variant()
    assert (v["mode"], v["order"], v["f32"]) == (V.TRANSLATE, order, int(f32_exact)), v
    if order == 2:  # (orders 1 and 3 have no pitched instantiation for every pixel type: the pick is the library's)
        assert (v["pitch"] > 0) == (pitch != 0), v
    assert c[0] == c[1] == c[2] >= 128, c  # every visit interior: the clean-path decision is reached at every visit
    return c, variant_has_clean_path(h)


def finite_counters(h, f32_exact, pitch, order=2):
    """Visit counters of the finite image (one item each and under a cap; no oracle: tests/test_gpu_persistent_sweep.py
    holds finite maps) -- they depend on the geometry only."""
    _, hs, large, hl = scene96(f32_exact)
    run = under(h, carrington_run(h, image("finite", f32_exact), hs, large, hl, LAGS, GRID, order), pitch=pitch)
    base = with_options(h, dict(OPTIONS, sweep_wgs=ONE_ITEM_EACH), run)
    c = counts(h)
    got = with_options(h, dict(OPTIONS, sweep_wgs=8), run)
    assert bitwise(got, base) and counts(h) == c and np.isfinite(base).all(), (c, counts(h))
    assert (np.asarray(h.last_counts()) == 65536).all()
    print(f"\n[persistent] finite image o{order} {'f32' if f32_exact else 'f64'} pitch {pitch}: counters {c}")
    return c, variant_has_clean_path(h)


# ---- 1. mixed dirty and clean visits in one item, and across the items of one workgroup ----------------------------------
@pytest.mark.parametrize("pitch", [0, -1], ids=["generic", "pitched"])
@pytest.mark.parametrize("f32_exact", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("pair", ["P", "Q"])
def test_complementary_pair(gpu_handle, pair, f32_exact, pitch):
    a, b = PAIRS[pair]
    for name in (a, b):  # (the precondition and the oracles' expectations: before the first GPU call)
        oracle_counts(name, f32_exact)
        oracle_map(name, f32_exact)
    c0, clean0 = finite_counters(gpu_handle, f32_exact, pitch)
    ca, clean_a = carrington(gpu_handle, a, f32_exact, pitch)
    cb, clean_b = carrington(gpu_handle, b, f32_exact, pitch)
    assert clean0 == clean_a == clean_b == (c0[3] == c0[2]), (clean0, clean_a, clean_b, c0)
    assert c0[:3] == ca[:3] == cb[:3], (c0, ca, cb)  # visits, lds, interior: geometry only
    print(f"[persistent] pair {pair}: all_finite {ca[3]} + {cb[3]}, interior {c0[2]}")
    if clean0:
        assert 0 < ca[3] < c0[2] and 0 < cb[3] < c0[2], (ca, cb, c0)
        assert ca[3] + cb[3] == c0[2], f"pair {pair}: all_finite {ca[3]} + {cb[3]} != interior {c0[2]}"
    else:
        assert c0[3] == ca[3] == cb[3] == 0, (c0, ca, cb)


def test_clean_path_off(gpu_handle):
    c, _ = carrington(gpu_handle, "P", True, 0, clean_path=0)
    assert c[3] == 0, c


@pytest.mark.parametrize("order", [1, 3])
def test_orders_1_and_3(gpu_handle, order):
    oracle_counts("P", True, order)
    c0, clean0 = finite_counters(gpu_handle, True, -1, order)
    c, clean = carrington(gpu_handle, "P", True, -1, order=order, caps=(8,))
    assert clean and clean0 and c0[3] == c0[2], (c0, c)
    assert c[:3] == c0[:3] and 0 < c[3] < c[2], (c0, c)
    assert 2 * c[3] == c[2], c  # (tile columns 0 and 2 dirty, 1 and 3 clean: half of the visits)


# ---- 2. methods that never take the clean path ---------------------------------------------------------------------------
def test_residus_methods(gpu_handle):
    from euispice_coreg_amd import _lib
    want_n = oracle_counts("Q", True)
    want = oracle_plain_residus("Q", True)
    ref, m = poisoned_case("Q", True)
    c, clean = carrington(gpu_handle, "Q", True, 0, method=_lib.METHOD_RESIDUS, want=want, want_n=want_n,
                          close=assert_masked, what="Q residus")
    assert not clean and c[3] == 0, c
    print(f"[persistent] masked residus on a poisoned reference: {m['poisoned'].min():.0f} ... {m['poisoned'].max():.0f} "
          f"poisoned terms a lag, {np.isfinite(m['masked']).sum()} lags with a number")
    c, clean = carrington(gpu_handle, "Q", True, 0, method=_lib.METHOD_RESIDUS_MASKED, want=m["masked"],
                          want_n=m["finite_terms"], close=assert_masked, large=ref, what="Q masked residus, poisoned")
    assert not clean and c[3] == 0, c


# ---- 3. the homography path ----------------------------------------------------------------------------------------------
HELIO_N = V.HELIO_INTERIOR_N
HELIO_T = 32
HELIO_X = {"H": 45, "H'": 80}          # NaN pixel column of each image
HELIO_DIRTY = {"H": 1, "H'": 2}        # the tile column whose interior tiles certainly stage it
HELIO_INTERIOR = ((0, 1), (0, 2), (1, 1), (1, 2))
HELIO_MARGIN = 0.01
HELIO_OPTIONS = dict(n_groups=16, tile_w=HELIO_T)


@functools.lru_cache(maxsize=None)
def helio_scene():
    sc = V.scene("helio-series", True, "interior")
    px = 1007.616 / HELIO_N
    lags = (17.0 + px * np.linspace(-0.5, 0.5, 13), -9.0 + px * np.linspace(-0.5, 0.5, 12), None, None,
            np.array([0.0, 0.3]))
    return sc["small"], sc["hs"], sc["large"], sc["hl"], lags


@functools.lru_cache(maxsize=None)
def helio_precondition():
    from oracle import coreg_oracle as O
    small, hs, large, hl, lags = helio_scene()
    assert small.shape == (HELIO_N, HELIO_N) and np.isfinite(small).all()
    st = H.oracle_state(small, hs, large, hl, lags, order=2)
    O.set_initial_header_values(st)
    O.prepare_reference(st, "helioprojective", None, True)
    table, shp = O.lag_table(st)
    assert table.shape[0] == 312 > 256  # two batches
    box = [[], [], [], []]
    k = HELIO_N // HELIO_T
    for lg in table:  # (every lag: a homography's box is not bounded by the corner lags')
        hdr = dict(st.hdr_small)
        O.shift_header(st, hdr, *lg)
        x, y = O.extract_coordinates_pixels(st.hdr_large, hdr, 2)
        for j, t in enumerate((np.asarray(x), np.asarray(y))):
            t = t.reshape(k, HELIO_T, k, HELIO_T)
            box[2 * j].append(t.min(axis=(1, 3)))
            box[2 * j + 1].append(t.max(axis=(1, 3)))
    xlo, xhi, ylo, yhi = (np.stack(a) for a in box)  # [lag, tile row, tile column]
    m = HELIO_MARGIN
    inside = (xlo >= m) & (xhi <= HELIO_N - 1 - m) & (ylo >= m) & (yhi <= HELIO_N - 1 - m)
    outside = (xlo < -m) | (xhi > HELIO_N - 1 + m) | (ylo < -m) | (yhi > HELIO_N - 1 + m)
    interior = np.zeros((k, k), dtype=bool)
    for ty, tx in HELIO_INTERIOR:
        interior[ty, tx] = True
    # a visit is interior when every lag of its batch is inside: certainly so, or certainly not, for any batch
    assert np.array_equal(inside.all(0), interior) and np.array_equal(outside.all(0), ~interior), (inside.all(0), outside.all(0))
    win = windows(xlo, xhi, APRON[2])
    for name, x in HELIO_X.items():
        for ty, tx in HELIO_INTERIOR:
            if tx == HELIO_DIRTY[name]:
                assert certainly_staged(x, win)[ty, tx], (name, ty, tx)
            else:
                assert certainly_not_staged(x, win)[ty, tx], (name, ty, tx)
    return True


@functools.lru_cache(maxsize=None)
def helio_case(name):
    helio_precondition()
    small, hs, large, hl, lags = helio_scene()
    img = np.array(small)
    if name != "finite":
        img[:, HELIO_X[name]] = np.nan
    want = H.oracle_helio(img, hs, large, hl, lags, order=2)
    m = M.sweep(H.oracle_state(img, hs, large, hl, lags, order=2), "helioprojective")
    n = m["finite_terms"]
    assert m["poisoned"].sum() == 0 and np.isfinite(want).all()
    if name != "finite":
        assert 0.9 * HELIO_N ** 2 < n.min() < n.max() < HELIO_N ** 2, (n.min(), n.max())
    for a in (img, want, n):
        a.setflags(write=False)
    return img, want, n


def helio(h, name):
    img, want, want_n = helio_case(name)
    _, hs, large, hl, lags = helio_scene()
    h.set_small(np.array(img))
    h.prepare_reference_helioprojective(large, hl, hs, 2)
    run = lambda: H.gpu_helio(h, img, hs, large, hl, lags, order=2, prepare=False)  # noqa: E731
    _, c, _ = three_ways_counts(h, run, want, want_n, 1e-7, f"helioprojective {name}", HELIO_OPTIONS)
    v = h.last_sweep_variant()
    assert v["order"] == 2 and v["mode"] in (V.HOMOGRAPHY, V.HOMOGRAPHY_SERIES), v
    return c, variant_has_clean_path(h)


def test_homography_path(gpu_handle):
    for name in ("finite", "H", "H'"):
        helio_case(name)
    c0, clean0 = helio(gpu_handle, "finite")
    ca, clean_a = helio(gpu_handle, "H")
    cb, clean_b = helio(gpu_handle, "H'")
    assert clean0 and clean_a and clean_b and c0[3] == c0[2], (c0, clean0, clean_a, clean_b)
    assert c0[:3] == ca[:3] == cb[:3] and 0 < c0[2] < c0[1], (c0, ca, cb)
    print(f"[persistent] helioprojective: all_finite {ca[3]} + {cb[3]}, interior {c0[2]}")
    assert 0 < ca[3] < c0[2] and 0 < cb[3] < c0[2], (ca, cb, c0)
    assert ca[3] + cb[3] == c0[2], (ca, cb, c0)


# ---- 4. bounded visits with masks under the queues -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def border_case():
    small, hs, large, hl, _ = H.scene(small_n=W, large_n=W, nan_frac=0.01)
    assert 0.005 * W * W < np.isnan(small).sum() < 0.02 * W * W
    c1 = np.concatenate([17.0 + PX * (np.arange(9) - 64.0), 17.0 + PX * (np.arange(9) - 4.0)])
    lags = (c1, -9.0 + PX * (np.arange(18) - 9.0), None, None, None)
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **V.BORDER_GRID)
    g = V.BORDER_GRID
    m = M.sweep(H.oracle_state(small, hs, large, hl, lags, order=2, shape=list(g["shape"]), lonlims=list(g["lonlims"]),
                               latlims=list(g["latlims"]), solar_r=(1.004,)), "carrington")
    n = m["finite_terms"]
    assert m["poisoned"].sum() == 0 and np.array_equal(n, m["count"])
    assert np.isfinite(want).any() and np.nanmin(n) < np.nanmax(n)
    for a in (small, large, want, n):
        a.setflags(write=False)
    return small, hs, large, hl, lags, want, n


def test_bounded_visits_with_masks(gpu_handle):
    small, hs, large, hl, lags, want, want_n = border_case()
    run = carrington_run(gpu_handle, small, hs, large, hl, lags, V.BORDER_GRID, 2)
    _, c, _ = three_ways_counts(gpu_handle, run, want, want_n, None, "bounded, 1 % NaN", dict(n_groups=24))
    assert 0 < c[0] and c[2] < c[0], c  # (visits under the bounds rule)
