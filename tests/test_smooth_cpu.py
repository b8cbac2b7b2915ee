"""
What of the NaN-aware smoothing runs without a GPU: the tables of a keyword (utils/smoothing.py: `smoothing_tables`), the
numpy oracle of the rule (tests/smooth_oracle.py) against scipy and against its own stated properties, and the keyword
checks of the public classes.
"""
import inspect
import math

import numpy as np
import pytest

from euispice_coreg_amd.pxlshift.alignment_pixels import smoothing_tables
from euispice_coreg_amd.utils.smoothing import MAX_R, check_table, gaussian_table
from tests import smooth_oracle as SO


# ---- smoothing_tables ---------------------------------------------------------------------------------------------------
def test_a_fwhm_becomes_a_normalised_gaussian_table():
    for fwhm in (0.5, 1.0, 3.0, 7.5, 37.0):
        sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        r = math.ceil(4.0 * sigma)
        w = gaussian_table(fwhm)
        assert w.dtype == np.float64 and w.shape == (2 * r + 1,) and abs(w.sum() - 1.0) <= len(w) * 2.0 ** -53
        assert np.array_equal(w, w[::-1]) and np.argmax(w) == r and np.all(w > 0)
        k = np.arange(-r, r + 1)
        assert np.allclose(w / w[r], np.exp(-k ** 2 / (2 * sigma ** 2)), rtol=1e-15, atol=0)
        # half the maximum at half the full width
        assert abs(np.interp(fwhm / 2, k, w / w[r]) - 0.5) < 0.02 or fwhm < 3


def test_argument_forms():
    assert smoothing_tables(None, "x") is None
    wy, wx = smoothing_tables(3.0, "x")
    assert np.array_equal(wy, wx) and np.array_equal(wy, gaussian_table(3.0))
    wy, wx = smoothing_tables(np.float32(3.0), "x")
    assert np.array_equal(wy, gaussian_table(3.0))
    wy, wx = smoothing_tables((2, 5.5), "x")
    assert np.array_equal(wy, gaussian_table(2.0)) and np.array_equal(wx, gaussian_table(5.5))
    ty, tx = np.array([1.0, 2.0, 1.0]), [0.0, 0.0, 1.0, 0.0, 3.0]
    wy, wx = smoothing_tables((ty, tx), "x")
    assert np.array_equal(wy, ty) and np.array_equal(wx, np.asarray(tx)) and wy is not ty  # as they are: not normalised
    wy, wx = smoothing_tables(([1.0], [1.0]), "x")
    assert np.array_equal(wy, [1.0]) and np.array_equal(wx, [1.0])


def test_fwhm_zero_is_the_identity_and_units_scale_a_fwhm():
    wy, wx = smoothing_tables((0, 3.0), "x")
    assert np.array_equal(wy, [1.0]) and len(wx) > 1
    assert all(np.array_equal(t, [1.0]) for t in smoothing_tables(0.0, "x"))
    wy, wx = smoothing_tables((8.0, 9.0), "x", scale=(0.25, 1.0 / 3.0))
    assert np.array_equal(wy, gaussian_table(2.0)) and np.array_equal(wx, gaussian_table(9.0 / 3.0))
    ty = np.array([1.0, 2.0, 1.0])
    assert np.array_equal(smoothing_tables((ty, ty), "x", scale=(0.5, 0.5))[0], ty)  # tables are not scaled


def test_the_reach_is_limited_and_says_so():
    sigma_to_fwhm = 2.0 * math.sqrt(2.0 * math.log(2.0))
    ok = 16.0 * sigma_to_fwhm * (1 - 1e-12)  # sigma just under 16: r = 64
    assert len(gaussian_table(ok)) == 2 * MAX_R + 1
    with pytest.raises(ValueError, match="r = 65.*64"):
        gaussian_table(16.01 * sigma_to_fwhm)
    with pytest.raises(ValueError, match="smooth_large.*64"):
        smoothing_tables((1.0, 500.0), "smooth_large")
    with pytest.raises(ValueError, match="64"):
        smoothing_tables(10.0, "x", scale=(10.0, 1.0))


@pytest.mark.parametrize("bad", ["gaussian", True, (1.0,), (1.0, 2.0, 3.0), -1.0, (1.0, -2.0), float("nan"), (float("inf"), 1.0),
                                 (np.ones(3), 2.0), (np.ones(2), np.ones(3)), (np.ones(131), np.ones(1)),
                                 (np.zeros(3), np.ones(1)), (np.array([1.0, np.nan, 1.0]), np.ones(1)),
                                 (np.array([1.0, -1.0, 1.0]), np.ones(1)), (np.ones((3, 3)), np.ones(3)), (True, 1.0),
                                 (np.zeros(0), np.ones(1))])
def test_bad_arguments_raise(bad):
    with pytest.raises(ValueError):
        smoothing_tables(bad, "x")


def test_check_table_limits():
    assert len(check_table(np.ones(129))) == 129 and len(check_table([2.0])) == 1
    for n in (0, 2, 128, 130, 131):
        with pytest.raises(ValueError):
            check_table(np.ones(n))


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def test_oracle_against_scipy_on_the_interior_of_a_finite_image():
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(3)
    v = rng.normal(0.0, 100.0, (61, 83))
    wy, wx = rng.uniform(0.1, 1.0, 9), rng.uniform(0.1, 1.0, 13)  # not symmetric, not normalised
    got = SO.smooth(v, wy, wx)
    want = correlate1d(correlate1d(v, wx, axis=1, mode="constant"), wy, axis=0, mode="constant") / (wy.sum() * wx.sum())
    inner = (slice(4, -4), slice(6, -6))
    scale = correlate1d(correlate1d(np.abs(v), wx, axis=1, mode="constant"), wy, axis=0, mode="constant") / (wy.sum() * wx.sum())
    assert np.all(np.abs(got[inner] - want[inner]) <= 64 * 2.0 ** -53 * scale[inner])
    assert np.isfinite(got).all()
    # the border renormalises like a hole: a constant image stays constant up to its rim
    flat = SO.smooth(np.full((20, 30), 7.0), wy, wx)
    assert np.all(np.abs(flat - 7.0) <= 1e-14)


def test_nan_in_gives_nan_out_at_the_same_pixels_only():
    rng = np.random.default_rng(4)
    v = rng.normal(10.0, 3.0, (40, 50))
    v[rng.random(v.shape) < 0.1] = np.nan
    v[5, 7], v[6, 7], v[20, :], v[:, 33] = np.inf, -np.inf, np.nan, np.nan
    v[10:17, 10:17] = np.nan
    v[13, 13] = 5.0  # an isolated finite pixel: its own value comes back
    w = gaussian_table(4.0)
    out = SO.smooth(v, w, w)
    assert np.array_equal(np.isnan(out), ~np.isfinite(v)) and not np.isinf(out).any()
    near = gaussian_table(1.0)  # reach 2: inside the block of NaN, three pixels to every side
    assert len(near) == 5 and abs(SO.smooth(v, near, near)[13, 13] - 5.0) <= 4 * 2.0 ** -53 * 5.0
    # a hole gives nothing to its neighbours: the result is that of any other value in the hole
    v2 = v.copy()
    v2[~np.isfinite(v)] = np.nan
    assert np.array_equal(SO.smooth(v2, w, w), out, equal_nan=True)
    # a table without centre weight: den = 0 at the isolated pixel gives NaN
    z = np.array([0.5, 0.0, 0.5])
    assert np.isnan(SO.smooth(v, z, z)[13, 13])


def test_the_identity_table_keeps_every_bit():
    rng = np.random.default_rng(5)
    v = rng.normal(0.0, 1.0, (33, 47)) * 10.0 ** rng.integers(-30, 30, (33, 47))
    v[3, 4], v[0, 0] = np.nan, -0.0
    out = SO.smooth(v, [1.0], [1.0])
    fin = np.isfinite(v)
    assert np.array_equal(out[fin].view(np.uint64) << 1, v[fin].view(np.uint64) << 1) and np.isnan(out[3, 4])
    assert np.array_equal(SO.smooth(v.astype(np.float32), [1.0], [1.0])[fin], v.astype(np.float32).astype(np.float64)[fin])


def test_the_bound_of_a_case_comes_from_its_own_reach():
    v = np.full((9, 9), -2.0)
    one, w = np.ones(1), gaussian_table(8.0)
    r = len(w) // 2
    assert np.allclose(SO.bound(v, one, one), 4 * 2 * 2.0 ** -53 * 2.0, rtol=1e-15)
    assert np.allclose(SO.bound(v, w, one), 4 * (2 * r + 2) * 2.0 ** -53 * 2.0, rtol=1e-12)


# ---- the keywords of the classes, without a GPU -------------------------------------------------------------------------
def _alignment(**kw):
    from euispice_coreg_amd.hdrshift import Alignment
    return Alignment("large.fits", "small.fits", [0.0], [0.0], None, None, None, **kw)


def test_alignment_checks_the_keywords_before_anything_is_loaded():
    A = _alignment()
    assert A.smooth_small is None and A.smooth_large is None and A.smooth_unit == "pixel"
    assert A._smoothing("small") is None and A._smoothing("large") is None
    with pytest.raises(ValueError, match="smooth_unit"):
        _alignment(smooth_small=3.0, smooth_unit="deg")
    with pytest.raises(ValueError, match="smooth_small"):
        _alignment(smooth_small="gaussian")
    with pytest.raises(ValueError, match="smooth_large"):
        _alignment(smooth_large=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="64"):
        _alignment(smooth_large=500.0)
    _alignment(smooth_large=500.0, smooth_unit="arcsec")  # (how many pixels that is: known once the header is)


def test_alignment_converts_arcsec_with_each_images_own_cdelt():
    A = _alignment(smooth_small=9.0, smooth_large=(8.8, 0.0), smooth_unit="arcsec")
    A.hdr_small = {"CDELT1": 3.0, "CDELT2": -1.5, "CUNIT1": "arcsec", "CUNIT2": "arcsec"}
    A.hdr_large = {"CDELT1": 4.4 / 3600.0, "CDELT2": 2.2 / 3600.0, "CUNIT1": "deg", "CUNIT2": "deg"}
    wy, wx = A._smoothing("small")
    assert np.allclose(wy, gaussian_table(6.0), rtol=1e-12) and np.allclose(wx, gaussian_table(3.0), rtol=1e-12)
    wy, wx = A._smoothing("large")
    assert np.allclose(wy, gaussian_table(4.0), rtol=1e-12) and np.array_equal(wx, [1.0])
    A.hdr_large = {"CDELT1": 4.4 / 3600.0, "CDELT2": 0.001 / 3600.0, "CUNIT1": "deg", "CUNIT2": "deg"}
    with pytest.raises(ValueError, match="smooth_large.*64"):
        A._smoothing("large")
    B = _alignment(smooth_small=(np.ones(3), np.ones(5)), smooth_unit="arcsec")
    B.hdr_small = A.hdr_small
    wy, wx = B._smoothing("small")
    assert len(wy) == 3 and len(wx) == 5  # tables are in pixels whatever the unit
    # the tables are part of the identity of a prepared reference
    C = _alignment(smooth_large=2.0)
    C.lonlims, C.latlims, C.shape, C.order = (0, 1), (0, 1), (4, 4), 2
    C._reference_tag = lambda frame, *what: (frame,) + tuple(tuple(np.ravel(w).tolist()) for w in what)
    plain = C._carrington_tag(1.004, None)
    C._smooth_large_tables = C._smoothing("large")
    assert C._carrington_tag(1.004, None) != plain and len(C._carrington_tag(1.004, None)) == len(plain) + 2


def test_the_other_classes_take_and_forward_the_keywords():
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    from euispice_coreg_amd.jitter_correction import jitter_correction as J
    S = AlignmentSpice("large.fits", "small.fits", [0.0], [0.0], smooth_small=2.0, smooth_large=(1.0, 3.0),
                       smooth_unit="arcsec")
    assert S.smooth_small == 2.0 and S.smooth_large == (1.0, 3.0) and S.smooth_unit == "arcsec"
    with pytest.raises(ValueError, match="smooth_unit"):
        AlignmentSpice("large.fits", "small.fits", [0.0], [0.0], smooth_unit="px")
    for fn in (J.jitter_correction_imagers, J._align_hrieuv_with_hrieuv):
        p = inspect.signature(fn).parameters
        assert p["smooth_small"].default is None and p["smooth_large"].default is None and p["smooth_unit"].default == "pixel"


def test_pxlshift_host_plan_holds_the_tables(tmp_path):
    from tests import pxlshift_cases as Cs
    A, kw = Cs.make("a", tmp_path)
    plan = A.host_plan(**kw)
    assert plan["smooth_large"] is None and plan["smooth_small"] is None and "bins_pending" not in plan
    plan = A.host_plan(**kw, smooth_large=3.0, smooth_small=(np.ones(1), np.array([1.0, 2.0, 1.0])))
    assert np.array_equal(plan["smooth_large"][0], gaussian_table(3.0)) and len(plan["smooth_small"][1]) == 3
    with pytest.raises(ValueError, match="smooth_large"):
        A.host_plan(**kw, smooth_large="gaussian")
    with pytest.raises(ValueError, match="64"):
        A.host_plan(**kw, smooth_small=400.0)
    # default bins are quantiles of the smoothed images: pending until the GPU has made them; given edges are not
    plan = A.host_plan(**kw, method="mutual_information", smooth_large=3.0)
    assert plan["bins"] is None and plan["bins_pending"] == 16
    with pytest.raises(ValueError, match="bins"):
        A.host_plan(**kw, method="mutual_information", smooth_large=3.0, bins=40)
    plan = A.host_plan(**kw, method="mutual_information", smooth_large=3.0, bins=([1.0, 2.0], [3.0]))
    assert "bins_pending" not in plan and len(plan["bins"][0]) == 2
    plan = A.host_plan(**kw, method="mutual_information", bins=8)
    assert "bins_pending" not in plan and len(plan["bins"][0]) == 7
    for fn in (A.find_best_parameters, A.find_local_shifts):
        p = inspect.signature(fn).parameters
        assert p["smooth_large"].default is None and p["smooth_small"].default is None
