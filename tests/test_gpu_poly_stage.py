"""
The last axis of a spline sample as a polynomial in its fraction (csrc/spline_last.hpp) in every evaluator of the sweep:
gather_o2 / gather_o3 and the order-1 branch of point_lag on the LDS window (interior and under the bounds rule) and the
global-memory gather, orders 1, 2 and 3, every frame the order has a compiled kernel for, float32 and float64 pixels.

Sizes: the smoke scene's (96^2 image, 160^2 reference, 72 x 64 Carrington grid); the plate-carree frame has no such scene
and takes the case table's (tests/sweep_variant_cases.py: 90 x 120 map, 40 x 48 reference); one 256 x 256 grid, so that a
workgroup makes several visits.

1. test_three_paths: one lag plane A of 3 x 3 lags a pixel apart, three sweeps --
     LDS, lags A:              visits whose (tile, lag) box is inside the image run the interior loop (interior > 0;
                               Carrington, inner grid: all of them);
     LDS, every visit bounded: the same samples of A under the bounds rule (interior == 0, lds > 0).  Carrington and
                               plate carree, whose grid lies inside the image: one more lag in the same batch, far
                               enough to take every (tile, lag) box out of the image (120 pixels of a 96-pixel image;
                               45 of the plate-carree map around the 40 x 48 reference).  Helioprojective frames,
                               whose grid IS the image (and whose series map refuses a lag that far): tile_w 128,
                               tiles of 96 x 8 points that span the image's width, so that no box is inside;
     use_lds 0, lags A:        the global-memory gather (lds == 0).
   Each is held to the oracle on A at the frame's bound (1e-10 Carrington, 1e-7 helioprojective frames) and the three to
   each other at 1e-12, the project's figure for "same sweep, another rounding order".  The instantiation is the one
   csrc/sweep_variant.hpp picks for (mode, order, pixel type, pitch 0), by the library's own header compiled on the host;
   no lag-point is re-evaluated (refined_lag_points == 0): the map is k_sweep's.
2. test_fraction_zero_and_just_below_one: helioprojective frame, unrotated header, lags of whole and half pixels through
   zero: coordinates come out as integers, a hair below them, and (the half-pixel lags) as integers + 1/2 -- the
   y-fraction of orders 1 and 3 at exactly 0 and at the last doubles below 1, of order 2 likewise at the half-pixel
   lags.  The precondition is asserted on the oracle's own coordinates (to wcslib's noise).  LDS and global-memory
   gather; map 1e-7, counts equal to the oracle's.
3. test_nan_and_inf_columns: a NaN pixel column and a +inf pixel column, 256 x 256 Carrington grid, eight visits an
   item: the per-lag sample counts equal the oracle's exactly (a sample that a non-finite tap did not poison, or one
   dropped for nothing, shows in them), map 1e-10, orders 1, 2, 3, automatic and per-visit pitch.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import masked_scores_oracle as M
from tests import sweep_variant_cases as V

pytestmark = pytest.mark.gpu

N = 96
PX = 1007.616 / N                  # arcsec per pixel of the 96^2 image (synthetic.make_scene)
GRID = dict(shape=(72, 64), lonlims=V.INNER_GRID["lonlims"], latlims=V.INNER_GRID["latlims"])
FAR_PIXELS = {"carrington": 120.0, "car": 45.0}
BOUNDED_TILE_W = 128               # helioprojective frames: tiles as wide as the image
AGREE = 1e-12
BOUND = {"carrington": 1e-10, "helio-series": 1e-7, "helio-exact": 1e-7, "car": 1e-7}
CASES = [(frame, order) for frame, (_, compiled, _, _) in V.FRAMES.items() for order in compiled]


@functools.lru_cache(maxsize=None)
def scene(frame, f32_exact):
    """small, hs, large, hl, lags A, lags A + the far one, number of CRVAL1 lags of A."""
    if frame == "car":
        sc = V.scene("car", f32_exact, "interior")
        small, hs, large, hl = sc["small"], sc["hs"], sc["large"], sc["hl"]
        step = abs(float(hs["CDELT1"]))
        c1, c2 = 0.009 + step * np.arange(-1.0, 2.0), -0.0035 + step * np.arange(-1.0, 2.0)
        far = c1[-1] + FAR_PIXELS[frame] * step
    else:
        small, hs, large, hl, _ = H.scene(small_n=N, large_n=160, nan_frac=0.0, float32_exact=f32_exact)
        c1, c2 = 17.0 + PX * np.arange(-1.0, 2.0), -9.0 + PX * np.arange(-1.0, 2.0)
        far = c1[-1] + FAR_PIXELS["carrington"] * PX
    assert np.isfinite(small).all()
    for a in (small, large):
        a.setflags(write=False)
    return small, hs, large, hl, (c1, c2, None, None, None), (np.append(c1, far), c2, None, None, None), c1.size


@functools.lru_cache(maxsize=None)
def oracle_map(frame, order, f32_exact):
    small, hs, large, hl, lags, _, _ = scene(frame, f32_exact)
    if frame == "carrington":
        want = H.oracle_carrington(small, hs, large, hl, lags, order=order, **GRID)
    elif frame == "car":
        want = H.oracle_helio(small, hs, large, hl, lags, order=order, parallelism=False, unit_lag="deg")
    else:
        want = H.oracle_helio(small, hs, large, hl, lags, order=order)
    assert np.isfinite(want).all()
    want.setflags(write=False)
    return want


def prepare(h, frame, order, small, hs, large, hl):
    """Uploads and prepares; returns sweep(lags, **options) -> map shaped like the lag set."""
    from euispice_coreg_amd import _lib
    h.set_small(np.array(small))
    grid = None
    if frame == "carrington":
        grid = _lib.Grid(GRID["lonlims"], GRID["latlims"], GRID["shape"])
        h.prepare_reference_carrington(np.array(large), hl, grid, 1.004, order)
    elif frame == "car":
        h.set_reference_on_grid(np.asarray(large, dtype=np.float32))
    else:
        h.prepare_reference_helioprojective(np.array(large), hl, hs, order)

    def sweep(lags, **options):
        ls = _lib.LagSet(*lags)
        try:
            for name, value in dict(V.FRAMES[frame][3], **options).items():
                h.set_option(name, value)
            if frame == "carrington":
                out = h.sweep_carrington(hs, grid, 1.004, ls, order=order)
            else:
                out = h.sweep_helioprojective(hl if frame == "car" else hs, hs, ls, order=order)
        finally:
            for name, value in dict(V.OPTION_DEFAULTS, tile_w=0).items():
                h.set_option(name, value)
        return out.reshape(ls.shape + (1,))

    return sweep


def check_variant(h, frame, order, f32_exact, what):
    """The instantiation the library's own pick names for (mode, order, pixel type, no residus, pitch 0)."""
    mode = V.FRAMES[frame][0]
    entries, picks = V.native_picks([(mode, order, int(f32_exact), 0, 0)])
    v = h.last_sweep_variant()
    assert v["index"] == picks[0], (what, v, picks)
    want = entries[picks[0]]
    assert want == (mode, order, f32_exact, mode != V.TRANSLATE, False, 0), (what, want)
    assert tuple(v[k] for k in V.FIELDS[1:]) == want, (what, v, want)
    assert h.last_stats()["small_is_f32"] == int(f32_exact), what
    assert h.last_visit_counts()["refined_lag_points"] == 0, what


# ---- 1. interior loop, bounds rule, global-memory gather: the same samples -------------------------------------------
@pytest.mark.parametrize("f32_exact", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("frame,order", CASES, ids=[f"{f}-o{o}" for f, o in CASES])
def test_three_paths(gpu_handle, frame, order, f32_exact):
    h = gpu_handle
    small, hs, large, hl, lags, lags_far, n1 = scene(frame, f32_exact)
    want = oracle_map(frame, order, f32_exact)
    name = f"{frame} o{order} {'f32' if f32_exact else 'f64'}"
    sweep = prepare(h, frame, order, small, hs, large, hl)

    interior = sweep(lags)
    check_variant(h, frame, order, f32_exact, f"{name}, interior")
    vc = h.last_visit_counts()
    print(f"\n[poly stage] {name}: lags A {vc}")
    assert h.last_stats()["used_lds"] == 1 and vc["interior"] > 0, vc
    if frame == "carrington":
        assert vc["interior"] == vc["lds"] == vc["visits"], vc

    if frame in FAR_PIXELS:
        bounded = sweep(lags_far)[:n1]
    else:
        bounded = sweep(lags, tile_w=BOUNDED_TILE_W)
    check_variant(h, frame, order, f32_exact, f"{name}, bounded")
    vc = h.last_visit_counts()
    print(f"[poly stage] {name}: bounded {vc}")
    assert vc["interior"] == 0 and vc["all_finite"] == 0 and vc["lds"] > 0, vc

    glob = sweep(lags, use_lds=0)
    check_variant(h, frame, order, f32_exact, f"{name}, global")
    vc = h.last_visit_counts()
    assert h.last_stats()["used_lds"] == 0 and vc["lds"] == 0 < vc["visits"], vc

    got = {"interior": interior, "bounded": bounded, "global": glob}
    d = {k: float(np.nanmax(np.abs(g - want))) for k, g in got.items()}
    pair = {f"{a}-{b}": float(np.nanmax(np.abs(got[a] - got[b])))
            for a, b in (("interior", "bounded"), ("interior", "global"), ("bounded", "global"))}
    print(f"[poly stage] {name}: against the oracle {d} (bound {BOUND[frame]:.0e}); among themselves {pair} (bound {AGREE:.0e})")
    for k, g in got.items():
        H.assert_corr_close(g, want, BOUND[frame], f"{name}, {k}")
    for k, v in pair.items():
        assert v <= AGREE, f"{name}: {k} differ by {v:.3e} > {AGREE:.0e}"


# ---- 2. the fraction at exactly 0 and at the last doubles below 1 -----------------------------------------------------
HALF_STEPS = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])


@functools.lru_cache(maxsize=None)
def unrotated_scene():
    """The 96^2 scene under a header without rotation (tests/test_gpu_fuzz.py: lags of whole pixels), its pixels PX."""
    small, hs, large, hl, _, _, _ = scene("helio-series", True)
    hs = dict(hs)
    hs.update(CROTA=0.0, PC1_1=1.0, PC1_2=0.0, PC2_1=0.0, PC2_2=1.0)
    lags = (HALF_STEPS * abs(hs["CDELT1"]), HALF_STEPS * abs(hs["CDELT2"]), None, None, None)
    return small, hs, large, hl, lags


@functools.lru_cache(maxsize=None)
def whole_pixel_case(order):
    """(oracle map, oracle counts) under HALF_LAGS, with the fractions the lags are there for asserted on the oracle's
    coordinates: the fraction scipy hands the weights (order 2: of c + 1/2) is within 1e-9 above 0 at some samples
    and within 1e-9 below 1 at others, under lags that keep the sample inside the image.  (The oracle's coordinates
    carry wcslib's rounding noise of ~1e-11 px about the integer; the sweep's own map of an unrotated whole-pixel lag
    is exact to a few ulp, so that its fractions are 0 itself and the last doubles below 1.)"""
    from oracle import coreg_oracle as O
    small, hs, large, hl, HALF_LAGS = unrotated_scene()
    st = H.oracle_state(small, hs, large, hl, HALF_LAGS, order=order)
    O.set_initial_header_values(st)
    O.prepare_reference(st, "helioprojective", None, True)
    table, _ = O.lag_table(st)
    zero = below = 0
    for lg in table:
        hdr = dict(st.hdr_small)
        O.shift_header(st, hdr, *lg)
        _, y = O.extract_coordinates_pixels(st.hdr_large, hdr, order)
        y = np.asarray(y, dtype=np.float64)
        y = y[(y >= 0.0) & (y <= N - 1.0)] + (0.5 if order == 2 else 0.0)
        f = y - np.floor(y)
        zero += int((f < 1e-9).sum())
        below += int((f > 1.0 - 1e-9).sum())
    assert zero > 0 and below > 0, (order, zero, below)
    want = H.oracle_helio(small, hs, large, hl, HALF_LAGS, order=order)
    m = M.sweep(H.oracle_state(small, hs, large, hl, HALF_LAGS, order=order), "helioprojective")
    assert np.isfinite(want).all() and m["poisoned"].sum() == 0
    for a in (want, m["count"]):
        a.setflags(write=False)
    return want, m["count"], zero, below


@pytest.mark.parametrize("order", [1, 2, 3])
def test_fraction_zero_and_just_below_one(gpu_handle, order):
    h = gpu_handle
    want, want_n, zero, below = whole_pixel_case(order)
    small, hs, large, hl, HALF_LAGS = unrotated_scene()
    sweep = prepare(h, "helio-series", order, small, hs, large, hl)
    for options in (dict(), dict(use_lds=0)):
        got = sweep(HALF_LAGS, **options)
        what = f"whole and half pixel lags, o{order}, {options}"
        check_variant(h, "helio-series", order, True, what)
        print(f"\n[poly stage] {what}: {zero} samples at fraction 0, {below} just below 1; "
              f"max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
        H.assert_corr_close(got, want, 1e-7, what)
        n = np.asarray(h.last_counts(), dtype=np.float64).reshape(np.shape(want_n))
        assert np.array_equal(n, np.asarray(want_n, dtype=np.float64)), what


# ---- 3. a NaN column and a +inf column, several visits an item -----------------------------------------------------------
GRID256 = dict(shape=(256, 256), lonlims=(237.0, 253.0), latlims=(-1.0, 11.0))
LAGS256 = (17.0 + 0.25 * PX * (np.arange(9) - 4), -9.0 + 0.25 * PX * (np.arange(9) - 4), None, None, None)
NAN_COLUMN, INF_COLUMN = 47, 65


@functools.lru_cache(maxsize=None)
def nonfinite_case(order):
    small, hs, large, hl, _, _, _ = scene("carrington", True)
    img = np.array(small)
    img[:, NAN_COLUMN] = np.nan
    img[:, INF_COLUMN] = np.inf
    want = H.oracle_carrington(img, hs, large, hl, LAGS256, order=order, **GRID256)
    m = M.sweep(H.oracle_state(img, hs, large, hl, LAGS256, order=order, shape=list(GRID256["shape"]),
                               lonlims=list(GRID256["lonlims"]), latlims=list(GRID256["latlims"]), solar_r=(1.004,)),
                "carrington")
    n = m["finite_terms"]
    assert m["poisoned"].sum() == 0 and np.array_equal(n, m["count"]) and np.isfinite(want).all()
    assert 0.8 * 65536 < n.min() < n.max() < 0.97 * 65536, (n.min(), n.max())  # both columns under the grid, counts vary
    for a in (img, want, n):
        a.setflags(write=False)
    return img, want, n


@pytest.mark.parametrize("pitch", [0, -1], ids=["generic", "pitched"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_nan_and_inf_columns(gpu_handle, order, pitch):
    from euispice_coreg_amd import _lib
    h = gpu_handle
    img, want, want_n = nonfinite_case(order)
    _, hs, large, hl, _, _, _ = scene("carrington", True)
    g = _lib.Grid(GRID256["lonlims"], GRID256["latlims"], GRID256["shape"])
    ls = _lib.LagSet(*LAGS256)
    h.set_small(np.array(img))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, order)
    options = dict(n_groups=8, tile_w=64, taper_frac=0, pitch=pitch)
    try:
        for name, value in options.items():
            h.set_option(name, value)
        got = h.sweep_carrington(hs, g, 1.004, ls, order=order).reshape(ls.shape + (1,))
    finally:
        for name, value in dict(n_groups=0, tile_w=0, taper_frac=-1, pitch=-1).items():
            h.set_option(name, value)
    what = f"NaN and inf columns, o{order}, pitch {pitch}"
    v, vc = h.last_sweep_variant(), h.last_visit_counts()
    print(f"\n[poly stage] {what}: variant {v}, {vc}, max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
    assert (v["mode"], v["order"], v["f32"], v["resid"]) == (V.TRANSLATE, order, 1, 0), v
    if pitch == 0:
        assert v["pitch"] == 0, v
    assert vc["refined_lag_points"] == 0, vc
    assert vc["visits"] >= 64 and vc["lds"] == vc["visits"], vc   # 64 tiles in 8 shares: eight visits an item
    assert 0 < vc["all_finite"] < vc["interior"], vc              # windows with and without the two columns
    H.assert_corr_close(got, want, 1e-10, what)
    n = np.asarray(h.last_counts(), dtype=np.float64).reshape(np.shape(want_n))
    assert np.array_equal(n, np.asarray(want_n, dtype=np.float64)), what
