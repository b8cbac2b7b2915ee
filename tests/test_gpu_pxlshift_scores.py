"""
GPU tests of the second score (`residus_masked`), the per-lag sample counts, `min_overlap` and
`return_type="PixelAlignmentResults"` of the pixel-lag alignment (pxlshift), against tests/pxlshift_scores_oracle.py run
on the object's own prepared images and `host_plan`.

Bounds: counts are compared exactly.  A score is within CARR_RTOL = 1e-10 of tests/test_gpu_masked_scores.py, per entry,
|got - want| <= 1e-10 |want|, with the same NaN pattern and the same best entry: a summation of n <= 9 000 non-negative
terms in another order moves it by at most n 2^-53 ~ 1e-12.  The Pearson coefficient keeps the bound of
tests/test_gpu_pxlshift.py (2^-23 |corr| + 1e-12: its numerator is rounded to float32).
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels, PixelAlignmentResults

from . import pxlshift_cases as Cs
from . import pxlshift_scores_oracle as S

pytestmark = pytest.mark.gpu

CARR_RTOL = 1e-10
CASES = ["a", "b", "c", "e", "d_crota"]
BAND = 2048  # small-image pixels staged per band (csrc/kernels_pixels.hpp: kPixTile), at most 64 rows


def _run(A, kw, method):
    cube = A.find_best_parameters(**kw, method=method)
    return cube, A.last_counts


def _check_masked(got, want, label):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print(label, "residus_masked: max relative error", err.max() if err.size else None)
    assert np.all(np.abs(got[fin] - want[fin]) <= CARR_RTOL * np.abs(want[fin]))
    if fin.any():
        assert np.nanargmin(got) == np.nanargmin(want)


def _check_corr(got, want, label):
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    d = np.abs(got - want)
    print(label, "correlation: max |diff|", np.nanmax(d))
    assert np.all(d[np.isfinite(want)] <= (2.0 ** -23 * np.abs(want) + 1e-12)[np.isfinite(want)])
    assert np.nanargmax(got) == np.nanargmax(want)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every case once: object, arguments, the oracle's cubes, (cube, counts) of either method."""
    out = {}
    for name in CASES:
        A, kw = Cs.make(name, tmp_path_factory.mktemp("pxs_" + name))
        o = S.scores(A.data_large, A.data_small, A.host_plan(**kw))
        out[name] = (A, kw, o, _run(A, kw, "correlation"), _run(A, kw, "residus_masked"))
    return out


def test_the_cases_walk_what_they_are_there_for(runs):
    h, w = runs["b"][0].data_small.shape
    assert -(-h // min(64, BAND // w)) == 5  # five row bands
    dx = np.asarray(runs["c"][1]["lag_dx"])
    assert (np.abs(np.diff(dx)) > 15).sum() == 4 and len(dx) == 6  # ragged groups: four of one lag, one of two
    assert len(runs["a"][1]["lag_drot"]) == 3  # three rotation planes


@pytest.mark.parametrize("name", CASES)
def test_counts_and_scores_against_the_oracle(name, runs):
    A, kw, o, (corr, n_corr), (masked, n_masked) = runs[name]
    assert n_corr.shape == corr.shape == n_masked.shape == masked.shape and n_corr.dtype == np.float64
    assert np.array_equal(n_corr, o["count"])
    assert np.array_equal(n_masked, o["finite_terms"])
    _check_masked(masked, o["masked"], name)
    _check_corr(corr, o["corr"], name)


@pytest.mark.parametrize("name", ["a", "d_crota"])
def test_method_correlation_is_the_default_call(name, runs):
    A, kw, _, (corr, _), _ = runs[name]
    assert np.array_equal(A.find_best_parameters(**kw), corr, equal_nan=True)


def test_poisoned_terms(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    A.data_large[27:30, 44:47] = -10.0
    o = S.scores(A.data_large, A.data_small, A.host_plan(**kw))
    masked, counts = _run(A, kw, "residus_masked")
    nan = np.isnan(masked)
    assert nan.sum() == 38 and np.array_equal(nan, np.isnan(o["masked"])) and np.array_equal(nan, o["poisoned"] > 0)
    assert np.array_equal(counts, o["finite_terms"])
    _check_masked(masked, o["masked"], "poisoned")
    corr, n_corr = _run(A, kw, "correlation")
    assert np.array_equal(n_corr, o["count"])
    _check_corr(corr, o["corr"], "poisoned")


def test_second_column_band():
    """A 3 x (band + 5) small image: the smallest shape at which the second column band and its G - 1 extra box columns
    are walked."""
    rng = np.random.default_rng(20)
    small = rng.uniform(1.0, 9.0, (3, BAND + 5))
    large = rng.uniform(1.0, 9.0, (9, BAND + 17))
    for img, n in ((small, 7), (large, 19)):
        img[rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)] = np.nan
    small[1, BAND + 2] = large[4, BAND + 9] = np.nan  # (inside the second band too)
    hdr = {"CDELT1": 1.0, "CDELT2": 1.0, "CUNIT1": "arcsec", "CUNIT2": "arcsec"}
    A = AlignmentPixels((large, dict(hdr)), 0, (small, dict(hdr)), 0)
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    p = A.host_plan(**kw)
    assert (p["ratio_res_1"], p["ratio_res_2"]) == (1.0, 1.0) and tuple(p["sub_shape"]) == large.shape
    o = S.scores(A.data_large, A.data_small, p)
    assert o["count"].max() < small.size and o["count"].min() > small.size - 40
    masked, n_masked = _run(A, kw, "residus_masked")
    corr, n_corr = _run(A, kw, "correlation")
    assert np.array_equal(n_corr, o["count"]) and np.array_equal(n_masked, o["finite_terms"])
    _check_masked(masked, o["masked"], "column bands")
    _check_corr(corr, o["corr"], "column bands")


def test_batching_invariance(runs):
    """Case b's residus_masked cube and counts in one call, and cut into three calls along dx times two along dy."""
    A, kw, _, _, (whole, n_whole) = runs["b"]
    dx, dy = np.asarray(kw["lag_dx"]), np.asarray(kw["lag_dy"])
    cols, ncols = [], []
    for sx in (slice(0, 7), slice(7, 12), slice(12, None)):
        parts = [_run(A, dict(kw, lag_dx=dx[sx], lag_dy=dy[sy]), "residus_masked") for sy in (slice(0, 9), slice(9, None))]
        cols.append(np.concatenate([c for c, _ in parts], axis=1))
        ncols.append(np.concatenate([n for _, n in parts], axis=1))
    assert np.array_equal(np.concatenate(cols, axis=0), whole, equal_nan=True)
    assert np.array_equal(np.concatenate(ncols, axis=0), n_whole)


def test_min_overlap(runs):
    A, kw, o, (corr, counts), (masked, n_masked) = runs["a"]
    assert counts.max() == 511
    low = counts < 0.9 * 511
    assert low.sum() == 70 and counts.size == 105
    for method, cube in (("correlation", corr), ("residus_masked", masked)):
        for mo in (0.9, 460):
            got = A.find_best_parameters(**kw, method=method, min_overlap=mo)
            want_nan = counts < (0.9 * 511 if mo == 0.9 else 460)
            assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], cube[~want_nan])
            assert np.array_equal(A.last_counts, counts)  # (the counts are those of the sweep, not of the floor)
    assert np.array_equal(counts < 460, low)
    with pytest.raises(ValueError):
        A.find_best_parameters(**kw, min_overlap=600)


def test_results_object(runs):
    A, kw, _, (corr, counts), (masked, n_masked) = runs["a"]
    arr, _ = Cs.golden()
    assert np.unravel_index(np.nanargmax(arr["a/corr"]), corr.shape) == (4, 1, 1)
    for method, cube, n, best in (("correlation", corr, counts, (4, 1, 1)), ("residus_masked", masked, n_masked, (4, 1, 2))):
        R = A.find_best_parameters(**kw, method=method, return_type="PixelAlignmentResults")
        assert isinstance(R, PixelAlignmentResults) and R.method == method
        assert R.best == ("max" if method == "correlation" else "min")
        assert R.max_index == best
        assert np.array_equal(R.corr, cube, equal_nan=True) and np.array_equal(R.n_samples, n)
        assert np.array_equal(R.lag_dx, kw["lag_dx"]) and np.array_equal(R.lag_dy, kw["lag_dy"])
        assert R.drot == kw["lag_drot"][best[2]] and R.unit_rot == kw["unit_rot"]
        print(method, "shift_pixels", R.shift_pixels, "fit", R.fit_info)
        assert np.all(np.isfinite(R.shift_pixels))
        assert abs(R.shift_pixels[0] - kw["lag_dx"][best[0]]) <= 1 and abs(R.shift_pixels[1] - kw["lag_dy"][best[1]]) <= 1
        assert R.return_corrected_header([0])["CRVAL1"] != A.hdr_small["CRVAL1"]


def test_last_counts_state(runs):
    A, kw = runs["c"][:2]
    with _lib.CoregHandle(0) as fresh:
        with pytest.raises(_lib.CoregError) as e:
            fresh.pixels_last_counts((1, 1, 1))
        assert e.value.code == _lib.COREG_ESTATE
    cube = A.find_best_parameters(**kw)
    hnd = _lib.shared_handle(-1 if A.device is None else A.device)
    assert np.array_equal(hnd.pixels_last_counts(cube.shape), A.last_counts)
    hnd.pixels_set_small(A.data_small)
    with pytest.raises(_lib.CoregError) as e:
        hnd.pixels_last_counts(cube.shape)
    assert e.value.code == _lib.COREG_ESTATE
    with pytest.raises(_lib.CoregError) as e:  # the library's own refusals of a method
        hnd.pixels_sweep(A.host_plan(**kw), _lib.METHOD_RESIDUS)
    assert e.value.code == _lib.COREG_ENOTIMPL
    with pytest.raises(_lib.CoregError) as e:
        hnd.pixels_sweep(A.host_plan(**kw), 7)
    assert e.value.code == _lib.COREG_EINVAL
