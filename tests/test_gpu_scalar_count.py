"""
k_sweep's bounded loop tests the bounds rule 0 <= n <= max with one unsigned compare of bit patterns per axis on the LDS
path of the translation (kernels_sweep.hpp point_lag), and its masked interior loop keeps the per-lane sample count under
the finite mask (the count on the scalar unit measured slower and was not built in: DESIGN.md section 4.4, round 8).
Per-lag counts and the map against the CPU oracles on the cases at which either loop can go wrong:

  interior geometry   image to align 96^2, reference 96^2, Carrington grid 64 x 64 (4 tiles) over the inner window of
                      tests/sweep_variant_cases.py, 5 x 5 whole-pixel lags about the pointing error, order 2, the generic
                      and the pitched kernel, the points cut in the fewest shares (a wave walks 128 samples in one visit).
                      Every visit is interior (asserted).
    1. no NaN, clean_path 0      the masked loop with every sample counted
    2. 0.5 % NaN pixels          sparse masks
    3. 15 % NaN pixels           3 in 4 samples lost
    4. a NaN block               as large as one lag's footprint: that lag counts exactly zero, its coefficient is NaN
  5. bounded visits   image to align 24^2 under 25 whole-pixel x 5 whole- and half-pixel lags that span it, so no visit is
                      interior (asserted); orders 1, 2, 3.  And the series homography on the helioprojective frame, whose
                      grid is the image: the zero lag puts samples on 0 and on W - 1, the whole- and half-pixel lags beside
                      it a pixel and half a pixel outside.

Counts equal the oracle's exactly: `finite_terms`, which on these scenes (reference > 0 everywhere: no poisoned term,
asserted) is `count`, the Pearson sums' sample count.  Interior maps: 1e-10 (CARR_RTOL; the coefficients are <= 1 in
size).  Bounded maps: the project's own bounds for these frames (tests/test_gpu_sweep_variants.py), 1e-9 on the
Carrington frame and 1e-7 on the helioprojective one -- the change touches no float64 operation of a sample.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import masked_scores_oracle as M
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import CARR_RTOL, assert_counts

pytestmark = pytest.mark.gpu

N = 96
PX = 1007.616 / N
GRID = dict(shape=(64, 64), lonlims=V.INNER_GRID["lonlims"], latlims=V.INNER_GRID["latlims"])
LAGS = (17.0 + PX * np.arange(-2, 3), -9.0 + PX * np.arange(-2, 3), None, None, None)
N_POINTS = 64 * 64


@functools.lru_cache(maxsize=None)
def base_scene():
    small, hs, large, hl, _ = H.scene(small_n=N, large_n=N, nan_frac=0.0)
    for a in (small, large):
        a.setflags(write=False)
    return small, hs, large, hl


def footprint(lag1, lag2):
    """Pixel box (x0, x1, y0, y1) of the grid under the lag (lag1, lag2) of LAGS."""
    from oracle import coreg_oracle as O
    small, hs, large, hl = base_scene()
    st = H.oracle_state(small, hs, large, hl, LAGS, shape=list(GRID["shape"]), lonlims=list(GRID["lonlims"]),
                        latlims=list(GRID["latlims"]), solar_r=(1.004,))
    O.set_initial_header_values(st)
    hdr = dict(st.hdr_small)
    O.shift_header(st, hdr, LAGS[0][lag1], LAGS[1][lag2], 0.0, 0.0, 0.0)
    nx, ny = O.carrington_coords(hdr, 1.004, list(GRID["shape"]), list(GRID["lonlims"]), list(GRID["latlims"]))
    # (the centre tap of a sample is the pixel nearest to it: a NaN there is enough at any order)
    return int(np.floor(np.nanmin(nx))), int(np.ceil(np.nanmax(nx))), int(np.floor(np.nanmin(ny))), int(np.ceil(np.nanmax(ny)))


@functools.lru_cache(maxsize=None)
def interior_case(kind):
    """(image to align, oracle map, oracle counts) of an interior case; computed once, never modified."""
    small, hs, large, hl = base_scene()
    img = small.copy()
    rng = np.random.default_rng(23)
    if kind == "sparse":
        img[rng.random(img.shape) < 0.005] = np.nan
    elif kind == "dense":
        img[rng.random(img.shape) < 0.15] = np.nan
    elif kind == "block":
        x0, x1, y0, y1 = footprint(0, 0)
        assert 0 <= x0 < x1 < N and 0 <= y0 < y1 < N, (x0, x1, y0, y1)  # (interior geometry: the footprint is inside)
        img[y0:y1 + 1, x0:x1 + 1] = np.nan
    else:
        assert kind == "finite"
    want = H.oracle_carrington(img, hs, large, hl, LAGS, **GRID)
    st = H.oracle_state(img, hs, large, hl, LAGS, shape=list(GRID["shape"]), lonlims=list(GRID["lonlims"]),
                        latlims=list(GRID["latlims"]), solar_r=(1.004,))
    m = M.sweep(st, "carrington")
    assert m["poisoned"].sum() == 0 and np.array_equal(m["finite_terms"], m["count"])
    for a in (img, want, m["finite_terms"]):
        a.setflags(write=False)
    return img, want, m["finite_terms"]


def run_carrington(h, img, hs, large, hl, lags, grid, order, **options):
    from euispice_coreg_amd import _lib
    g = _lib.Grid(grid["lonlims"], grid["latlims"], grid["shape"])
    ls = _lib.LagSet(*lags)
    h.set_small(np.array(img))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, order)
    try:
        for name, value in options.items():
            h.set_option(name, value)
        out = h.sweep_carrington(hs, g, 1.004, ls, order=order)
    finally:
        h.set_option("clean_path", 1)
        h.set_option("pitch", -1)
        h.set_option("n_groups", 0)
    return out.reshape(ls.shape + (1,)), h.last_counts().reshape(ls.shape + (1,)), h.last_visit_counts()


def check_interior(h, kind, pitch, what, **options):
    _, hs, large, hl = base_scene()
    img, want, counts = interior_case(kind)
    # (n_groups 8, the fewest: the 4096 points are cut in 8 shares of 512, a wave walks 128 samples in one visit; the
    # default cuts a grid this small in 256 shares of one chunk per wave)
    got, n, vc = run_carrington(h, img, hs, large, hl, LAGS, GRID, 2, pitch=pitch, n_groups=8, **options)
    v = h.last_sweep_variant()
    print(f"\n[scalar count] {what}: {vc}, kernel {v}, max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}, "
          f"samples lost {N_POINTS - n.min():.0f} at most")
    assert (v["mode"], v["order"], v["resid"]) == (V.TRANSLATE, 2, False) and (v["pitch"] > 0) == (pitch != 0), v
    assert vc["interior"] == vc["lds"] == vc["visits"] > 0, vc  # every visit runs the interior loop
    assert_counts(n, counts, what)
    H.assert_corr_close(got, want, CARR_RTOL, what)
    return n, vc


PITCHES = pytest.mark.parametrize("pitch", [0, -1], ids=["generic", "pitched"])


@PITCHES
def test_all_finite_image_through_the_masked_loop(gpu_handle, pitch):
    n, vc = check_interior(gpu_handle, "finite", pitch, "all finite, clean_path 0", clean_path=0)
    assert vc["all_finite"] == 0 and (n == N_POINTS).all(), vc  # the masked loop ran and counted every sample
    _, vc = check_interior(gpu_handle, "finite", pitch, "all finite, clean path")
    assert vc["all_finite"] == vc["interior"], vc  # (the per-chunk count of the clean path, as before)


@PITCHES
def test_sparse_nan(gpu_handle, pitch):
    n, vc = check_interior(gpu_handle, "sparse", pitch, "0.5 % NaN")
    assert vc["all_finite"] < vc["interior"] and (n < N_POINTS).all() and (n > 0.9 * N_POINTS).all(), (vc, n.min())


@PITCHES
def test_dense_nan(gpu_handle, pitch):
    n, vc = check_interior(gpu_handle, "dense", pitch, "15 % NaN")
    assert vc["all_finite"] == 0 and (n < 0.4 * N_POINTS).all() and (n > 0).all(), (vc, n.min(), n.max())


@PITCHES
def test_one_lag_loses_every_sample(gpu_handle, pitch):
    n, _ = check_interior(gpu_handle, "block", pitch, "NaN block")
    _, want, _ = interior_case("block")
    # (the lag at the other corner of the lag plane is shifted by four pixels: a strip of its samples misses the block)
    assert n[0, 0, 0] == 0 and np.isnan(want[0, 0, 0, 0, 0, 0]), n.ravel()
    assert n[4, 4, 0] > 100 and np.isfinite(want[4, 4, 0, 0, 0, 0]), n.ravel()


# ---- 5. bounded visits ------------------------------------------------------------------------------------------------
NB = 24
PXB = 1007.616 / NB
B_LAGS = (17.0 + PXB * np.arange(-12, 13), -9.0 + PXB * np.array([-12.0, -0.5, 0.0, 0.5, 12.0]), None, None, None)
B_GRID = dict(shape=(40, 36), lonlims=H.CARR_LON, latlims=H.CARR_LAT)


@functools.lru_cache(maxsize=None)
def bounded_scene():
    small, hs, large, hl, _ = H.scene(small_n=NB, large_n=N, nan_frac=0.01)
    for a in (small, large):
        a.setflags(write=False)
    return small, hs, large, hl


@pytest.mark.parametrize("order", [1, 2, 3])
def test_bounded_visits_carrington(gpu_handle, order):
    small, hs, large, hl = bounded_scene()
    want = H.oracle_carrington(small, hs, large, hl, B_LAGS, order=order, **B_GRID)
    st = H.oracle_state(small, hs, large, hl, B_LAGS, order=order, shape=list(B_GRID["shape"]),
                        lonlims=list(B_GRID["lonlims"]), latlims=list(B_GRID["latlims"]), solar_r=(1.004,))
    m = M.sweep(st, "carrington")
    assert m["poisoned"].sum() == 0
    for pitch in (0, -1):
        what = f"bounded, order {order}, pitch {pitch}"
        got, n, vc = run_carrington(gpu_handle, small, hs, large, hl, B_LAGS, B_GRID, order, pitch=pitch)
        v = gpu_handle.last_sweep_variant()
        print(f"\n[scalar count] {what}: {vc}, kernel {v}, max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
        assert (v["mode"], v["order"]) == (V.TRANSLATE, order), v
        assert vc["interior"] == 0 < vc["lds"] == vc["visits"], vc  # the lags span the image: the bounds rule everywhere
        assert_counts(n, m["finite_terms"], what)
        assert n.min() < n.max() and n.max() > 0  # (the rule does cut: the lags differ in what they keep)
        H.assert_corr_close(got, want, 1e-9, what)


def test_bounded_visits_homography_series(gpu_handle):
    sc = V.scene("helio-series", True, "border")
    small, hs, large, hl = sc["small"], sc["hs"], sc["large"], sc["hl"]
    lags = (V.PX1 * np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), V.PX2 * np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), None, None, None)
    want = H.oracle_helio(small, hs, large, hl, lags, order=2)
    m = M.sweep(H.oracle_state(small, hs, large, hl, lags, order=2), "helioprojective")
    assert m["poisoned"].sum() == 0
    h = gpu_handle
    try:
        h.set_option("pitch", 0)
        got = H.gpu_helio(h, small, hs, large, hl, lags, order=2)
    finally:
        h.set_option("pitch", -1)
    v, vc = h.last_sweep_variant(), h.last_visit_counts()
    print(f"\n[scalar count] bounded, series homography: {vc}, kernel {v}, max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
    assert (v["mode"], v["order"]) == (V.HOMOGRAPHY_SERIES, 2), v
    assert vc["lds"] > vc["interior"], vc  # the grid is the image: its outer tiles reach the edge at every lag
    assert_counts(h.last_counts(), m["finite_terms"], "bounded, series homography")
    H.assert_corr_close(got, want, 1e-7, "bounded, series homography")
