"""CPU tests of the masked residus' host side: the numpy oracle (tests/masked_scores_oracle.py) on the scenes the GPU tests
use, `min_overlap` on plain arrays (hdrshift.alignment.apply_min_overlap), `AlignmentResults(best="min")`, and the keywords
that carry the three through the classes."""
import inspect
import json
import os

import numpy as np
import pytest

from oracle import coreg_oracle as O
from tests import helpers as H
from tests import masked_scores_oracle as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# CRVAL1 lags 17 + (-600 ... 600 step 150) arcsec on the small scene of tests/helpers.py: the grid slides off the image
WIDE_LAGS = (17.0 + np.arange(-600.0, 601.0, 150.0), [-9.0], None, None, None)
WIDE_COUNTS = [448, 560, 671, 786, 782, 778, 779, 702, 580]


def carr_state(lags, shape=(48, 40), lon=H.CARR_LON, lat=H.CARR_LAT, **scene_kw):
    small, hs, large, hl, _ = H.scene(**scene_kw)
    return H.oracle_state(small, hs, large, hl, lags, shape=list(shape), lonlims=list(lon), latlims=list(lat),
                          solar_r=(1.004,))


# ---- the oracle -----------------------------------------------------------------------------------------------------
def test_oracle_on_the_usual_carrington_grid():
    """Where the reference's residus is NaN at every lag-point, the masked one is a number, with 780 ... 788 of the 1920
    grid points behind it and no poisoned term."""
    lags = (17.0 + 2.0 * (np.arange(5) - 2), -9.0 + 2.0 * (np.arange(5) - 2), None, None, None)
    r = M.sweep(carr_state(lags), "carrington")
    assert np.isfinite(r["masked"]).all() and r["masked"].shape == (5, 5, 1, 1, 1, 1)
    assert r["count"].min() == 780 and r["count"].max() == 788 and r["poisoned"].sum() == 0
    assert np.isnan(O.find_best_header_parameters(carr_state(lags), "carrington", method="residus")).all()


def test_oracle_equals_the_unmasked_residus_at_full_overlap():
    lags = (17.0 + 2.0 * (np.arange(3) - 1), -9.0 + 2.0 * (np.arange(3) - 1), None, None, None)
    kw = dict(shape=(40, 36), lon=(243.0, 249.0), lat=(2.0, 8.0), nan_frac=0.0)
    r = M.sweep(carr_state(lags, **kw), "carrington")
    want = O.find_best_header_parameters(carr_state(lags, **kw), "carrington", method="residus")
    assert np.array_equal(r["masked"], want) and (r["count"] == 1440).all()


def test_oracle_counts_of_the_wide_lags():
    r = M.sweep(carr_state(WIDE_LAGS), "carrington")
    assert r["count"].ravel().astype(int).tolist() == WIDE_COUNTS
    m = r["masked"].ravel()
    # the 448-sample lag-point is the second-best residus: a score without its count misleads
    assert np.argsort(m)[:2].tolist() == [4, 0] and abs(m[0] - 9.70) < 0.01 and abs(m[4] - 9.39) < 0.01


def test_oracle_poisoned_term_and_empty_mask():
    a = np.array([4.0, 9.0, 0.0, np.nan, 16.0])
    b = np.array([3.0, np.nan, 1.0, 2.0, 12.0])
    n, score, bad = M.masked_terms(a, b)
    assert (n, bad) == (3, 1) and np.isnan(score)  # (0 - 1) / sqrt(0) = -inf: np.std gives NaN
    n, score, bad = M.masked_terms(a[[0, 4]], b[[0, 4]])
    assert (n, bad) == (2, 0) and score == np.std([0.5, 1.0])
    n, score, bad = M.masked_terms(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))
    assert (n, bad) == (0, 0) and np.isnan(score)
    assert np.isnan(M.masked_terms(np.array([-4.0, 4.0]), np.array([1.0, 1.0]))[1])  # sqrt of a negative reference


# ---- min_overlap ----------------------------------------------------------------------------------------------------
def test_min_overlap_on_plain_arrays():
    from euispice_coreg_amd.hdrshift.alignment import apply_min_overlap
    counts = np.array(WIDE_COUNTS, dtype=np.float64).reshape(9, 1)
    corr = np.arange(9.0).reshape(9, 1)
    assert apply_min_overlap(corr, counts, None) is corr
    # a fraction of the largest finite count: exactly the entries with at least 0.9 x 786 samples, four of nine
    got = apply_min_overlap(corr, counts, 0.9)
    keep = counts >= 0.9 * 786
    assert keep.sum() == 4 and np.array_equal(np.isfinite(got), keep) and np.array_equal(got[keep], corr[keep])
    assert np.array_equal(corr.ravel(), np.arange(9.0))  # (the input is left alone)
    # a count
    got = apply_min_overlap(corr, counts, 700)
    assert np.array_equal(np.isfinite(got).ravel(), np.array(WIDE_COUNTS) >= 700) and np.isfinite(got).sum() == 5
    assert np.isfinite(apply_min_overlap(corr, counts, np.int64(1))).all()
    # a lag-point that was never evaluated (NaN count) goes, and does not enter the largest count
    c2 = counts.copy()
    c2[3] = np.nan
    got = apply_min_overlap(corr, c2, 0.9)
    assert np.array_equal(np.isfinite(got).ravel(), np.nan_to_num(c2.ravel()) >= 0.9 * 782)
    # entries that were NaN stay NaN
    c3 = corr.copy()
    c3[4] = np.nan
    assert np.isnan(apply_min_overlap(c3, counts, 1)[4])


@pytest.mark.parametrize("bad", [0, -3, 1.0, 0.0, 1.5, -0.2, True, "0.5", [1], float("nan")])
def test_min_overlap_refuses_anything_else(bad):
    from euispice_coreg_amd.hdrshift import Alignment
    from euispice_coreg_amd.hdrshift.alignment import apply_min_overlap
    with pytest.raises(ValueError):
        apply_min_overlap(np.zeros(3), np.ones(3), bad)
    with pytest.raises(ValueError):  # at construction, before anything is loaded
        Alignment("a.fits", "b.fits", [0.0], [0.0], None, None, None, min_overlap=bad)


def test_min_overlap_that_leaves_nothing_says_so():
    from euispice_coreg_amd.hdrshift.alignment import apply_min_overlap
    with pytest.raises(ValueError, match="leaves no lag-point"):
        apply_min_overlap(np.arange(9.0), np.array(WIDE_COUNTS, dtype=float), 787)
    with pytest.raises(ValueError, match="leaves no lag-point"):
        apply_min_overlap(np.arange(3.0), np.full(3, np.nan), 0.5)
    with pytest.raises(ValueError, match="shape"):
        apply_min_overlap(np.arange(3.0), np.ones(4), 1)


# ---- AlignmentResults(best="min") -------------------------------------------------------------------------------------
def bowl(centre=(4.3, 5.6), shape=(9, 11)):
    """A residus-like map: about 0.8 at a non-integer minimum, a few units away from it."""
    x, y = np.meshgrid(np.arange(float(shape[0])), np.arange(float(shape[1])), indexing="ij")
    return 0.8 + 3.0 * (1.0 - np.exp(-((x - centre[0]) ** 2 / 7.0 + (y - centre[1]) ** 2 / 9.0)))


@pytest.mark.parametrize("fit", ["native", "scipy"])
def test_best_min_is_best_max_on_the_flipped_rescaled_map(fit):
    from euispice_coreg_amd.hdrshift import AlignmentResults
    b = bowl()[:, :, None, None, None, None]
    l1, l2 = np.arange(9.0) * 1.5 - 6.0, np.arange(11.0) * 0.5 - 3.0
    n = np.arange(b.size, dtype=np.float64).reshape(b.shape)
    lo = AlignmentResults(b, l1, l2, None, None, None, "arcsec", fit=fit, n_samples=n, best="min")
    assert tuple(int(v) for v in lo.max_index) == (4, 6, 0, 0, 0, 0) == np.unravel_index(np.argmin(b), b.shape)
    assert lo.best == "min" and lo.n_samples is n and lo.corr is not None and np.array_equal(lo.corr, b)
    z = (b.max() - b) / (b.max() - b.min())
    hi = AlignmentResults(z, l1, l2, None, None, None, "arcsec", fit=fit)
    assert hi.best == "max" and hi.n_samples is None
    assert tuple(lo.shift_pixels) == tuple(hi.shift_pixels) and tuple(lo.shift_arcsec) == tuple(hi.shift_arcsec)
    # and the fit finds the bowl's centre between the lag-points
    assert abs(lo.shift_pixels[0] - 4.3) < 0.05 and abs(lo.shift_pixels[1] - 5.6) < 0.05
    assert abs(lo.shift_arcsec[0] - (4.3 * 1.5 - 6.0)) < 0.08 and abs(lo.shift_arcsec[1] - (5.6 * 0.5 - 3.0)) < 0.03


def test_best_min_ignores_nan_and_falls_back_to_the_argmin():
    from euispice_coreg_amd.hdrshift import AlignmentResults
    b = bowl()[:, :, None, None, None, None].copy()
    b[0, 0] = np.nan  # (a lag-point min_overlap took out, far from the minimum)
    r = AlignmentResults(b, np.arange(9.0), np.arange(11.0), None, None, None, "arcsec", best="min")
    assert tuple(int(v) for v in r.max_index)[:2] == (4, 6) and abs(r.shift_pixels[0] - 4.3) < 0.05
    # a NaN inside the fit's 5 x 5 patch: the argmin, where a correlation map falls back to the argmax
    b[5, 6] = np.nan
    with pytest.warns(UserWarning, match="Gaussian fitting failed"):
        r = AlignmentResults(b, np.arange(9.0), np.arange(11.0), None, None, None, "arcsec", best="min")
    assert tuple(r.shift_pixels) == (4, 6, 0, 0, 0) and tuple(r.shift_arcsec) == (4.0, 6.0, 0.0, 0.0, 0.0)
    # a flat map: nothing to rescale by -- the argmin again
    with pytest.warns(UserWarning, match="Gaussian fitting failed"):
        r = AlignmentResults(np.full((5, 5, 1, 1, 1, 1), 2.0), np.arange(5.0), np.arange(5.0), None, None, None, "arcsec",
                             best="min")
    assert tuple(r.shift_pixels) == (0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        AlignmentResults(b, np.arange(9.0), np.arange(11.0), None, None, None, "arcsec", best="smallest")


def test_best_max_is_unchanged_on_the_reference_fixture():
    """The default still gives what the reference's object gave on results_5d_golden (argmax, fitted shift)."""
    from euispice_coreg_amd.hdrshift import AlignmentResults
    g = np.load(os.path.join(GOLDEN, "results_5d_golden.npz"))
    with open(os.path.join(GOLDEN, "results_5d_golden.json")) as f:
        cases = json.load(f)["cases"]
    for name, c in sorted(cases.items()):
        ax = [np.asarray(a) for a in c["axes"]]
        args = (g[f"case/{name}/corr"], ax[0], ax[1], ax[2], ax[3], ax[4], c["unit_lag"])
        R = AlignmentResults(*args, best="max", n_samples=None)
        assert [int(v) for v in R.max_index] == c["max_index"]
        assert np.allclose(np.asarray(R.shift_pixels, dtype=float), c["shift_pixels"], rtol=0,
                           atol=1e-2 if "edge" in name else 2e-3)
        D = AlignmentResults(*args)
        assert tuple(D.shift_pixels) == tuple(R.shift_pixels) and tuple(D.shift_arcsec) == tuple(R.shift_arcsec)


# ---- the keywords through the classes ---------------------------------------------------------------------------------
def test_method_names_and_codes():
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.hdrshift.alignment import library_method
    assert (_lib.METHOD_CORRELATION, _lib.METHOD_RESIDUS, _lib.METHOD_RESIDUS_MASKED) == (0, 1, 2)
    assert [library_method(n) for n in ("correlation", "residus", "residus_masked")] == [0, 1, 2]
    with pytest.raises(NotImplementedError):  # alignment.py:549
        library_method("masked")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "coreg_hip.h")) as f:
        hdr = f.read()
    assert "#define COREG_METHOD_RESIDUS_MASKED 2" in hdr
    assert "int coreg_last_counts(coreg_handle* h, double* dst, int dst_on_device);" in hdr
    assert "int coreg_multi_last_counts(coreg_multi* m, double* dst_host);" in hdr


def test_keywords_reach_the_classes():
    from euispice_coreg_amd.hdrshift import (Alignment, AlignmentResults, AlignmentSpice,
                                             AlignementSpiceIterativeContextRaster)
    from euispice_coreg_amd.jitter_correction import jitter_correction as J
    for cls in (Alignment, AlignmentSpice, AlignementSpiceIterativeContextRaster):
        assert inspect.signature(cls.__init__).parameters["min_overlap"].default is None
    p = inspect.signature(AlignmentResults.__init__).parameters
    assert p["n_samples"].default is None and p["best"].default == "max"
    for fn in (J.jitter_correction_imagers, J._align_hrieuv_with_hrieuv):
        p = inspect.signature(fn).parameters
        assert p["method"].default == "correlation" and p["min_overlap"].default is None
    A = Alignment("a.fits", "b.fits", [0.0], [0.0], None, None, None, min_overlap=0.5)
    assert A.min_overlap == 0.5 and A.last_counts is None
    # the minimum is the best entry of residus_masked alone: `residus` keeps the reference's argmax
    for method, best in (("correlation", "max"), ("residus", "max"), ("residus_masked", "min")):
        A.method = method
        assert A._results_keywords()["best"] == best
