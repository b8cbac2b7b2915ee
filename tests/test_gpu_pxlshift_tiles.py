"""
GPU tests of the local shift field of the pixel-lag alignment (`AlignmentPixels.find_local_shifts`,
coreg_pixels_sweep_tiles): one lag cube and count cube per tile of the small image, against
tests/pxlshift_tiles_oracle.py run on the object's own prepared images and `host_plan`, and against the untiled sweep.

Bounds, those of tests/test_gpu_pxlshift_scores.py: counts are compared exactly; `residus_masked` per entry within
CARR_RTOL = 1e-10 relative, the Pearson coefficient within 2^-23 |corr| + 1e-12 (its numerator is rounded to float32);
the same NaN pattern and the same best entry per tile.  A tile of the whole image, the tiles next to a changed one and a
cube cut into several calls are compared bit for bit.

The shapes are the smallest that walk each path (csrc/kernels_pixels.hpp: a band is at most 2048 pixels and 64 rows, its
shape that of the nominal tile): ragged last tiles on both axes, a tile of two column bands, a tile of two row bands.
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels, LocalShiftField

from . import pxlshift_cases as Cs
from . import pxlshift_tiles_cases as TC
from . import pxlshift_tiles_oracle as T

pytestmark = pytest.mark.gpu

CARR_RTOL = 1e-10
METHODS = ("correlation", "residus_masked")
TILES = {"a": (10, 9), "b": (40, 50), "c": (10, 9)}  # 25 x 21, 70 x 130, 25 x 21 pixels: ragged on both axes
BAND = 2048


def _local(A, kw, tile_shape, method, **more):
    """The raw cubes of a tiled call: (corr, n_samples, field)."""
    F = A.find_local_shifts(**kw, tile_shape=tile_shape, method=method, sub_lag=False, min_fill=0.0, **more)
    assert isinstance(F, LocalShiftField) and F.corr.dtype == F.n_samples.dtype == np.float64
    return F.corr, F.n_samples, F


def _check(got, want, method, label, ties=False):
    """Every tile's cube against the oracle's: the bound of the method, the NaN pattern, the best entry per tile.
    ties: tiles of one to three pixels hold entries that are equal by construction (two points correlate at +-1 whatever
    the lag); there another best entry passes when the oracle's own scores of the two lie within twice the bound."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), label
    fin = np.isfinite(want)
    d = np.abs(got[fin] - want[fin])
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 if method == "correlation" else CARR_RTOL * np.abs(want)
    with np.errstate(all="ignore"):
        rel = d / np.abs(want[fin])
    print(label, method, "max |diff|", d.max() if d.size else None, "max relative", np.nanmax(rel) if d.size else None)
    assert np.all(d <= bound[fin])
    arg = np.nanargmax if method == "correlation" else np.nanargmin
    for ty in range(want.shape[0]):
        for tx in range(want.shape[1]):
            if np.isfinite(want[ty, tx]).any():
                g, w = arg(got[ty, tx]), arg(want[ty, tx])
                if ties and g != w:
                    wt = want[ty, tx].ravel()
                    assert abs(wt[g] - wt[w]) <= 2 * bound[ty, tx].ravel()[w], (label, ty, tx)
                else:
                    assert g == w, (label, ty, tx)


def _oracle_keys(method):
    return ("corr", "count") if method == "correlation" else ("masked", "finite_terms")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Cases a, b, c once: object, arguments, the tiled oracle, and per method (tiled cubes, tiled counts, untiled cube,
    untiled counts)."""
    out = {}
    for name, ts in TILES.items():
        A, kw = Cs.make(name, tmp_path_factory.mktemp("pxt_" + name))
        o = T.scores(A.data_large, A.data_small, A.host_plan(**kw), ts)
        per = {}
        for m in METHODS:
            cube = A.find_best_parameters(**kw, method=m)
            counts = A.last_counts
            per[m] = _local(A, kw, ts, m)[:2] + (cube, counts)
        out[name] = (A, kw, o, per)
    return out


def test_the_cases_walk_what_they_are_there_for(runs):
    for name, (th, tw) in TILES.items():
        h, w = runs[name][0].data_small.shape
        assert h % th and w % tw and h > th and w > tw  # ragged last tiles on both axes, more than one tile
    assert len(runs["a"][1]["lag_drot"]) == 3  # three rotation planes
    dx = np.asarray(runs["c"][1]["lag_dx"])
    assert (np.abs(np.diff(dx)) > 15).sum() == 4 and len(dx) == 6  # ragged dx groups


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(TILES))
def test_against_the_oracle(name, method, runs):
    A, kw, o, per = runs[name]
    corr, counts = per[method][:2]
    key, nkey = _oracle_keys(method)
    assert corr.shape == counts.shape == o[key].shape
    assert np.array_equal(counts, o[nkey])
    _check(corr, o[key], method, f"{name} tiles {TILES[name]}")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(TILES))
def test_one_tile_of_the_whole_image_is_the_untiled_sweep(name, method, runs):
    A, kw, _, per = runs[name]
    cube, counts = per[method][2:]
    corr, n, F = _local(A, kw, A.data_small.shape, method)
    assert corr.shape == (1, 1) + cube.shape
    assert np.array_equal(corr[0, 0], cube, equal_nan=True) and np.array_equal(n[0, 0], counts)  # bit for bit
    assert F.tile_slices == [[(slice(0, A.data_small.shape[0]), slice(0, A.data_small.shape[1]))]]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(TILES))
def test_counts_of_the_tiles_sum_to_the_untiled_counts(name, method, runs):
    _, _, _, per = runs[name]
    assert np.array_equal(per[method][1].sum(axis=(0, 1)), per[method][3])


def _plain(large, small):
    return AlignmentPixels((large, dict(TC.HDR)), 0, (small, dict(TC.HDR)), 0)


def test_a_tile_wider_than_a_band():
    """The 3 x (band + 5) image of test_gpu_pxlshift_scores.py::test_second_column_band in tiles of (2, band + 2): a tile
    of a second column band (2 columns wide, one row per band), a ragged 3-column tile and ragged 1-row tiles."""
    rng = np.random.default_rng(20)
    small = rng.uniform(1.0, 9.0, (3, BAND + 5))
    large = rng.uniform(1.0, 9.0, (9, BAND + 17))
    for img, n in ((small, 7), (large, 19)):
        img[rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)] = np.nan
    small[1, BAND + 2] = large[4, BAND + 9] = np.nan  # (inside the second band too)
    A = _plain(large, small)
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    ts = (2, BAND + 2)
    o = T.scores(A.data_large, A.data_small, A.host_plan(**kw), ts)
    assert o["count"].shape == (2, 2, 5, 3, 1) and o["count"][1, 1].max() <= 3 and o["count"][0, 0].min() > 2 * BAND - 40
    for m in METHODS:
        corr, n, _ = _local(A, kw, ts, m)
        key, nkey = _oracle_keys(m)
        assert np.array_equal(n, o[nkey])
        _check(corr, o[key], m, "column bands", ties=True)


def test_a_tile_taller_than_a_band():
    """A 70 x 5 image in tiles of (67, 3): 64 rows, then a second row band of 3, inside a tile; ragged tiles of 3 rows and
    of 2 columns."""
    rng = np.random.default_rng(21)
    small = rng.uniform(1.0, 9.0, (70, 5))
    large = rng.uniform(1.0, 9.0, (78, 13))
    for img, n in ((small, 6), (large, 9)):
        img[rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)] = np.nan
    small[65, 1] = np.nan  # (inside the second row band too)
    A = _plain(large, small)
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-2, 3), lag_drot=np.array([0.0]))
    ts = (67, 3)
    assert ts[0] > 64 and ts[0] * ts[1] <= BAND  # the rows of a band, not its pixels, end the first band
    o = T.scores(A.data_large, A.data_small, A.host_plan(**kw), ts)
    assert o["count"].shape == (2, 2, 5, 5, 1) and o["count"][0, 0].max() > 64 * 3
    for m in METHODS:
        corr, n, _ = _local(A, kw, ts, m)
        key, nkey = _oracle_keys(m)
        assert np.array_equal(n, o[nkey])
        _check(corr, o[key], m, "row bands", ties=True)


def test_an_all_nan_tile(runs, tmp_path):
    """Tile (0, 1) of case a without a finite pixel (unrotated planes: a rotation would carry the NaN into its
    neighbours): its entries are NaN, its counts 0, it is not valid; every other tile keeps its bits."""
    A0, kw0, _, _ = runs["a"]
    kw = dict(kw0, lag_drot=np.array([0.0]))
    A, _ = Cs.make("a", tmp_path)
    A.data_small[0:10, 9:18] = np.nan
    for m in METHODS:
        before, n_before, _ = _local(A0, kw, (10, 9), m)
        F = A.find_local_shifts(**kw, tile_shape=(10, 9), method=m, sub_lag=False)
        assert np.isnan(F.corr[0, 1]).all() and not F.n_samples[0, 1].any()
        assert not F.valid[0, 1] and F.valid.sum() == 8
        assert np.isnan(F.shift_dx[0, 1]) and np.isnan(F.best_score[0, 1]) and (F.best_index[0, 1] == -1).all()
        other = np.ones((3, 3), dtype=bool)
        other[0, 1] = False
        assert np.isfinite(before[0, 1]).all()
        assert np.array_equal(F.corr[other], before[other], equal_nan=True)
        assert np.array_equal(F.n_samples[other], n_before[other])


def test_a_poisoned_block(runs, tmp_path):
    """Pixels <= 0 of the large image that every lag keeps under tile (0, 0): with residus_masked only that tile's lags
    over the block become NaN, as the oracle's; the correlation keeps such pixels."""
    A0, kw, _, per = runs["a"]
    A, _ = Cs.make("a", tmp_path)
    A.data_large[30:32, 38:40] = -10.0
    o = T.scores(A.data_large, A.data_small, A.host_plan(**kw), (10, 9))
    hit = o["poisoned"] > 0
    assert hit[0, 0].sum() == 51 and hit.sum() == 51  # 51 of the 105 lags of tile (0, 0), no other tile
    masked, n, _ = _local(A, kw, (10, 9), "residus_masked")
    assert np.array_equal(np.isnan(masked), hit) and np.array_equal(n, o["finite_terms"])
    _check(masked, o["masked"], "residus_masked", "poisoned")
    other = ~hit.any(axis=(2, 3, 4))
    assert np.array_equal(masked[other], per["residus_masked"][0][other])  # the other tiles: bit for bit
    corr, n, _ = _local(A, kw, (10, 9), "correlation")
    assert np.isfinite(corr).all() and np.array_equal(n, o["count"])
    _check(corr, o["corr"], "correlation", "poisoned")


def test_batching_invariance(runs):
    """Case b's tiled residus_masked cubes and counts in one call, and cut into three calls along dx times two along dy."""
    A, kw, _, per = runs["b"]
    whole, n_whole = per["residus_masked"][:2]
    dx, dy = np.asarray(kw["lag_dx"]), np.asarray(kw["lag_dy"])
    cols, ncols = [], []
    for sx in (slice(0, 7), slice(7, 12), slice(12, None)):
        parts = [_local(A, dict(kw, lag_dx=dx[sx], lag_dy=dy[sy]), TILES["b"], "residus_masked")[:2]
                 for sy in (slice(0, 9), slice(9, None))]
        cols.append(np.concatenate([c for c, _ in parts], axis=3))
        ncols.append(np.concatenate([n for _, n in parts], axis=3))
    assert np.array_equal(np.concatenate(cols, axis=2), whole, equal_nan=True)
    assert np.array_equal(np.concatenate(ncols, axis=2), n_whole)


def test_two_drift_scene():
    A, kw, ts, want = TC.two_drift_object()
    want = np.array(want)
    for m in METHODS:
        F = A.find_local_shifts(**kw, tile_shape=ts, method=m, sub_lag=True)
        print(m, "dx", F.shift_dx.tolist(), "dy", F.shift_dy.tolist(), "fitted", F.fitted.tolist(), "scores",
              F.best_score.tolist())
        assert F.valid.all() and F.corr.shape == (2, 2, 9, 9, 1)
        best_dx, best_dy = kw["lag_dx"][F.best_index[..., 0]], kw["lag_dy"][F.best_index[..., 1]]
        assert np.array_equal(best_dx, want[..., 0]) and np.array_equal(best_dy, want[..., 1])
        assert np.isfinite(F.shift_dx).all() and np.isfinite(F.shift_dy).all()
        assert np.all(np.abs(F.shift_dx - best_dx) <= 1) and np.all(np.abs(F.shift_dy - best_dy) <= 1)
        assert np.isfinite(F.median_shift).all() and np.isfinite(F.scatter).all()
        assert F.drift().shape == (2, 3) and np.all(F.drot == 0.0)
        assert "4 valid of 4 tiles" in str(F)
        A.find_best_parameters(**kw, method=m)
        assert np.array_equal(F.n_samples.sum(axis=(0, 1)), A.last_counts)
    assert np.nanmax(A.find_best_parameters(**kw)) < 0.6  # no single lag fits the image


def _code(fn, *args, **kw):
    with pytest.raises(_lib.CoregError) as e:
        fn(*args, **kw)
    return e.value.code


def test_state_and_refusals(runs):
    A, kw = runs["c"][:2]
    plan = A.host_plan(**kw, tile_shape=(10, 9))
    shape5 = plan["tile_grid"] + (len(plan["lag_dx"]), len(plan["lag_dy"]), len(plan["lag_drot"]))
    with _lib.CoregHandle(0) as hnd:
        assert _code(hnd.pixels_last_tile_counts, shape5) == _lib.COREG_ESTATE  # a fresh handle
        hnd.pixels_set_large(A.data_large)
        hnd.pixels_set_small(A.data_small)
        cube = hnd.pixels_sweep(plan, plan["method_code"])
        assert _code(hnd.pixels_last_tile_counts, shape5) == _lib.COREG_ESTATE  # after an untiled sweep
        counts = hnd.pixels_last_counts(cube.shape)
        tiles = hnd.pixels_sweep_tiles(plan, plan["method_code"])
        assert tiles.shape == shape5
        assert _code(hnd.pixels_last_counts, cube.shape) == _lib.COREG_ESTATE  # after a tiled sweep
        n = hnd.pixels_last_tile_counts(shape5)
        assert np.array_equal(n.sum(axis=(0, 1)), counts)
        assert set(hnd.pixels_last_timing()) == {"prepare_ms", "pass0_ms", "pass1_ms"}
        hnd.pixels_set_small(A.data_small)
        assert _code(hnd.pixels_last_tile_counts, shape5) == _lib.COREG_ESTATE  # after a new image
        h, w = A.data_small.shape
        for bad in ((0, 9), (10, 0), (h + 1, 9), (10, w + 1), (-3, 9)):
            assert _code(hnd.pixels_sweep_tiles, plan, plan["method_code"], tile_shape=bad) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_tiles, plan, _lib.METHOD_RESIDUS) == _lib.COREG_ENOTIMPL
        assert _code(hnd.pixels_sweep_tiles, plan, 7) == _lib.COREG_EINVAL
        # 300 x 300 tiles of one pixel: more than 65535 planes x tiles, refused before any kernel runs
        big = _plain(np.ones((310, 310)), np.ones((300, 300)))
        bplan = big.host_plan([0], [0], [0.0], tile_shape=(1, 1))
        assert bplan["tile_grid"] == (300, 300)
        hnd.pixels_set_large(big.data_large)
        hnd.pixels_set_small(big.data_small)
        assert _code(hnd.pixels_sweep_tiles, bplan, bplan["method_code"]) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_last_tile_counts, (1,)) == _lib.COREG_ESTATE
