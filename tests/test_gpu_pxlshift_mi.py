"""
GPU tests of the mutual-information score of the pixel-lag alignment (`method="mutual_information"`, `bins=`,
coreg_pixels_set_bins), untiled and tiled, against tests/pxlshift_mi_oracle.py run on the
device's own prepared images (`A._rotated(k)`, `A._large_box()`, which tests/test_gpu_pxlshift.py pins): the bins are then
those of identical pixels, and a flip at an edge cannot hide in a tolerance.

Bounds: counts are compared exactly.  A score: |got - want| <= 1e-11 absolute, the same NaN pattern, the same argmax.  The
histogram is exact, so what remains is the logarithm, three roundings per term and a sum of at most 1 024 terms; with
sum n_ij / n = 1 and log B <= 3.5 that is at most about 1024 * 3.5 * 2^-53 ~ 4e-13, a factor of 25 inside the bound.
Measured on one MI355X: at most 8.9e-16 over the cases of this file.  Re-cut cubes, a tile of the whole image, the tiles
next to an all-NaN one and the other scores after this one are compared bit for bit.
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels, LocalShiftField, PixelAlignmentResults

from . import pxlshift_cases as Cs
from . import pxlshift_mi_oracle as M
from .pxlshift_tiles_cases import HDR
from .test_pxlshift_mi_cpu import scene_object

pytestmark = pytest.mark.gpu

MI = "mutual_information"
ATOL = 1e-11
CASES = ["a", "b", "c", "e"]
BINS = ["B2", "B16", "B32", "E1", "E31", "E16"]
BAND = 2048  # small-image pixels staged per band (csrc/kernels_pixels.hpp: kPixTile), at most 64 rows
worst = {"err": 0.0}


def _bins(A, key):
    """An integer B, or explicit lists per image: of 1 entry (the medians), of 31 entries (evenly spaced between the 2nd
    and the 98th percentile), or of 16 and 15 entries -- 17 x 16 cells, the first size above the 16 x 16 of B = 16 at which
    the library runs its workgroups of 512 threads (csrc/kernels_pixels_mi.hpp: kPixMiWideBytes)."""
    if key[0] == "B":
        return int(key[1:])
    out = []
    for img, n16 in ((A.data_small, 16), (A.data_large, 15)):
        v = img[np.isfinite(img)]
        n = {"E1": 1, "E31": 31, "E16": n16}[key]
        out.append(np.array([np.median(v)]) if n == 1 else np.linspace(*np.percentile(v, [2, 98]), n + 2)[1:-1])
        assert len(out[-1]) == n
    return tuple(out)


def _device_images(A, n_rot):
    return [A._rotated(k) for k in range(n_rot)], A._large_box()


def _check(got, want, n_got, n_want, label):
    assert got.shape == want.shape == n_got.shape and got.dtype == n_got.dtype == np.float64, label
    assert np.array_equal(n_got, n_want), label
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    worst["err"] = max(worst["err"], err)
    print(label, "mutual information: max |diff|", err, "largest so far", worst["err"])
    assert err <= ATOL, label
    lead = got.reshape(-1, *got.shape[-3:]) if got.ndim == 5 else got[None]
    ref = want.reshape(-1, *want.shape[-3:]) if want.ndim == 5 else want[None]
    for g, w in zip(lead, ref):  # (per tile, or the one cube)
        if np.isfinite(w).any():
            assert np.nanargmax(g) == np.nanargmax(w), label


def _close(got, want, n_got, n_want):
    """Counts, NaN pattern and bound, and the argmax up to ties (tiles of a few pixels, where most lags tie exactly at 0 or
    log 2 and either side may pick any of them): the oracle's entry at the device's argmax is the oracle's maximum to within
    twice the bound, which is the same argmax wherever the oracle's maximum leads by more than that."""
    assert np.array_equal(n_got, n_want) and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= ATOL)
    for g, w in zip(got.reshape(-1, *got.shape[-3:]), want.reshape(-1, *want.shape[-3:])):
        if np.isfinite(w).any():
            assert w.ravel()[np.nanargmax(g)] >= np.nanmax(w) - 2 * ATOL


def _sweep(A, kw, bins):
    cube = A.find_best_parameters(**kw, method=MI, bins=bins)
    return cube, A.last_counts


def _local(A, kw, tile_shape, bins, **more):
    F = A.find_local_shifts(**kw, tile_shape=tile_shape, method=MI, bins=bins, sub_lag=False, min_fill=0.0, **more)
    assert isinstance(F, LocalShiftField) and F.method == MI and F.best == "max"
    return F.corr, F.n_samples, F


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    return {name: Cs.make(name, tmp_path_factory.mktemp("pxmi_" + name)) for name in CASES}


def test_the_cases_walk_what_they_are_there_for(objects):
    h, w = objects["b"][0].data_small.shape
    assert -(-h // min(64, BAND // w)) == 5  # five row bands
    dx = np.asarray(objects["c"][1]["lag_dx"])
    assert (np.abs(np.diff(dx)) > 15).sum() == 4 and len(dx) == 6  # ragged groups: four of one lag, one of two
    a = objects["a"]
    assert len(a[1]["lag_drot"]) == 3 and np.isnan(a[0].data_small).any()  # three rotation planes, NaN pixels
    assert type(objects["e"][0]).__name__ == "AlignmentSpicePixel"


@pytest.mark.parametrize("key", BINS)
@pytest.mark.parametrize("name", CASES)
def test_against_the_oracle(name, key, objects):
    A, kw = objects[name]
    bins = _bins(A, key)
    got, n = _sweep(A, kw, bins)
    plan = A.host_plan(**kw, method=MI, bins=bins)
    planes, box = _device_images(A, len(plan["lag_drot"]))
    o = M.scores(None, A.data_small, plan, planes=planes, box=box)
    assert o["count"].max() > 0
    _check(got, o["mi"], n, o["count"], f"{name} {key}")
    t = A.last_timing
    assert set(t) == {"prepare_ms", "pass0_ms", "pass1_ms"} and t["pass0_ms"] > 0.0 and t["pass1_ms"] >= 0.0


def _second_band_pair():
    rng = np.random.default_rng(20)
    small = rng.uniform(1.0, 9.0, (3, BAND + 5))
    large = rng.uniform(1.0, 9.0, (9, BAND + 17))
    for img, n in ((small, 7), (large, 19)):
        img[rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)] = np.nan
    small[1, BAND + 2] = large[4, BAND + 9] = np.nan  # (inside the second band too)
    small[2, 7], large[3, 30] = np.inf, -np.inf  # kept: the end bins
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    return AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0), kw


def test_second_column_band():
    """A 3 x (band + 5) small image: the smallest shape at which the second column band and its G - 1 extra box columns
    are walked; an infinite pixel in either image."""
    A, kw = _second_band_pair()
    got, n = _sweep(A, kw, 16)
    plan = A.host_plan(**kw, method=MI, bins=16)
    planes, box = _device_images(A, 1)
    assert np.isinf(planes[0]).sum() == 1 and np.isinf(box).sum() == 1
    o = M.scores(None, A.data_small, plan, planes=planes, box=box)
    assert o["count"].max() < A.data_small.size and o["count"].min() > A.data_small.size - 40
    _check(got, o["mi"], n, o["count"], "column bands")


def test_a_constant_image_fills_one_cell():
    """300 x 300 equal pixels: 90 000 pairs in one counter (more than 16 bits hold), a score of exactly 0.0."""
    A = AlignmentPixels((np.full((310, 310), 5.0), dict(HDR)), 0, (np.full((300, 300), 5.0), dict(HDR)), 0)
    kw = dict(lag_dx=np.arange(-1, 2), lag_dy=np.array([0, 2]), lag_drot=np.array([0.0]))
    assert [len(e) for e in A.host_plan(**kw, method=MI)["bins"]] == [1, 1]
    got, n = _sweep(A, kw, None)
    assert got.shape == (3, 2, 1) and np.all(got == 0.0) and not np.signbit(got).any() and np.all(n == 90000.0)
    corr, nt, _ = _local(A, kw, (300, 300), None)
    assert np.all(corr == 0.0) and np.all(nt == 90000.0)


# ------------------------------------------------------------------------------------------------------------- tiles
def test_case_a_in_ragged_tiles(objects):
    A, kw = objects["a"]
    ts = (10, 9)
    corr, n, F = _local(A, kw, ts, 16)
    plan = A.host_plan(**kw, method=MI, bins=16, tile_shape=ts)
    planes, box = _device_images(A, 3)
    o = M.scores(None, A.data_small, plan, planes=planes, box=box, tile_shape=ts)
    assert corr.shape == (3, 3, 7, 5, 3)
    _check(corr, o["mi"], n, o["count"], "a tiles (10, 9)")
    cube, counts = _sweep(A, kw, 16)
    assert np.array_equal(n.sum(axis=(0, 1)), counts)  # the tiles' counts sum to the untiled ones
    whole, n_whole, _ = _local(A, kw, A.data_small.shape, 16)
    assert whole.shape == (1, 1) + cube.shape
    assert np.array_equal(whole[0, 0], cube, equal_nan=True) and np.array_equal(n_whole[0, 0], counts)  # bit for bit


def test_a_tile_wider_than_a_band():
    A, kw = _second_band_pair()
    ts = (2, BAND + 2)
    corr, n, _ = _local(A, kw, ts, 8)
    plan = A.host_plan(**kw, method=MI, bins=8, tile_shape=ts)
    planes, box = _device_images(A, 1)
    o = M.scores(None, A.data_small, plan, planes=planes, box=box, tile_shape=ts)
    assert o["count"].shape == (2, 2, 5, 3, 1) and o["count"][1, 1].max() <= 3 and o["count"][0, 0].min() > 2 * BAND - 40
    # (tiles of one to three pixels: every lag scores 0 or log 2 there; the argmax is asked of the two large tiles)
    _check(corr[:, :1], o["mi"][:, :1], n[:, :1], o["count"][:, :1], "column bands, tiled")
    _close(corr, o["mi"], n, o["count"])


def test_a_tile_taller_than_a_band():
    rng = np.random.default_rng(21)
    small = rng.uniform(1.0, 9.0, (70, 5))
    large = rng.uniform(1.0, 9.0, (78, 13))
    for img, k in ((small, 6), (large, 9)):
        img[rng.integers(0, img.shape[0], k), rng.integers(0, img.shape[1], k)] = np.nan
    small[65, 1] = np.nan  # (inside the second row band too)
    A = AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0)
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-2, 3), lag_drot=np.array([0.0]))
    ts = (67, 3)
    corr, n, _ = _local(A, kw, ts, 4)
    plan = A.host_plan(**kw, method=MI, bins=4, tile_shape=ts)
    planes, box = _device_images(A, 1)
    o = M.scores(None, A.data_small, plan, planes=planes, box=box, tile_shape=ts)
    assert o["count"].shape == (2, 2, 5, 5, 1) and o["count"][0, 0].max() > 64 * 3
    _check(corr[:1], o["mi"][:1], n[:1], o["count"][:1], "row bands, tiled")
    _close(corr, o["mi"], n, o["count"])


def test_an_all_nan_tile(objects, tmp_path):
    """Tile (0, 1) of case a without a number (unrotated planes; the bins of the unchanged image): NaN entries, counts of
    0, not valid; every other tile keeps its bits."""
    A0, kw0 = objects["a"]
    kw = dict(kw0, lag_drot=np.array([0.0]))
    bins = A0.host_plan(**kw, method=MI, bins=16)["bins"]
    before, n_before, _ = _local(A0, kw, (10, 9), bins)
    A, _ = Cs.make("a", tmp_path)
    A.data_small[0:10, 9:18] = np.nan
    F = A.find_local_shifts(**kw, tile_shape=(10, 9), method=MI, bins=bins, sub_lag=False)
    assert np.isnan(F.corr[0, 1]).all() and not F.n_samples[0, 1].any()
    assert not F.valid[0, 1] and F.valid.sum() == 8
    other = np.ones((3, 3), dtype=bool)
    other[0, 1] = False
    assert np.isfinite(before[0, 1]).all()
    assert np.array_equal(F.corr[other], before[other], equal_nan=True)
    assert np.array_equal(F.n_samples[other], n_before[other])


# ------------------------------------------------------------------------------------------------------------- re-cuts
def test_batching_invariance(objects):
    """Case b's cube and counts in one call, and cut into three calls along dx times two along dy: untiled and tiled."""
    A, kw = objects["b"]
    dx, dy = np.asarray(kw["lag_dx"]), np.asarray(kw["lag_dy"])
    for run, ax in ((lambda k: _sweep(A, k, 16), 0), (lambda k: _local(A, k, (40, 50), 16)[:2], 2)):
        whole, n_whole = run(kw)
        cols, ncols = [], []
        for sx in (slice(0, 7), slice(7, 12), slice(12, None)):
            parts = [run(dict(kw, lag_dx=dx[sx], lag_dy=dy[sy])) for sy in (slice(0, 9), slice(9, None))]
            cols.append(np.concatenate([c for c, _ in parts], axis=ax + 1))
            ncols.append(np.concatenate([n for _, n in parts], axis=ax + 1))
        assert np.array_equal(np.concatenate(cols, axis=ax), whole, equal_nan=True)
        assert np.array_equal(np.concatenate(ncols, axis=ax), n_whole)


# ------------------------------------------------------------------------------------------------------------- state
def test_the_other_scores_keep_their_bits(objects):
    A, kw = objects["a"]
    before = {}
    for m in ("correlation", "residus_masked"):
        before[m] = (A.find_best_parameters(**kw, method=m), A.last_counts)
    _sweep(A, kw, 32)
    _local(A, kw, (10, 9), 32)
    for m in ("correlation", "residus_masked"):
        assert np.array_equal(A.find_best_parameters(**kw, method=m), before[m][0], equal_nan=True)
        assert np.array_equal(A.last_counts, before[m][1])


def test_min_overlap_and_results_object(objects):
    A, kw = objects["a"]
    cube, counts = _sweep(A, kw, 16)
    assert counts.max() == 511 and (counts < 460).sum() == 70
    got = A.find_best_parameters(**kw, method=MI, bins=16, min_overlap=460)
    assert np.array_equal(np.isnan(got), counts < 460) and np.array_equal(got[counts >= 460], cube[counts >= 460])
    assert np.array_equal(A.last_counts, counts)
    with pytest.raises(ValueError):
        A.find_best_parameters(**kw, method=MI, min_overlap=600)
    R = A.find_best_parameters(**kw, method=MI, bins=16, return_type="PixelAlignmentResults")
    assert isinstance(R, PixelAlignmentResults) and R.method == MI and R.best == "max"
    assert R.max_index == np.unravel_index(np.nanargmax(cube), cube.shape)
    assert np.array_equal(R.corr, cube, equal_nan=True) and np.array_equal(R.n_samples, counts)
    assert np.all(np.isfinite(R.shift_pixels))


def test_the_scene_end_to_end():
    """The scene of tests/test_pxlshift_mi_cpu.py: the sweep finds the injected lag (-2, 3), every tile of (12, 10) does,
    and the destretch about that shift leaves the image where it is."""
    A, kw, bins = scene_object()
    cube, counts = _sweep(A, kw, bins)
    o = M.scores(A.data_large, A.data_small, A.host_plan(**kw, method=MI, bins=bins))
    _check(cube, o["mi"], counts, o["count"], "scene")
    top = np.sort(cube.ravel())[::-1]
    best = np.unravel_index(np.nanargmax(cube), cube.shape)
    assert (kw["lag_dx"][best[0]], kw["lag_dy"][best[1]]) == (-2, 3) and top[0] - top[1] >= 0.3
    corr = A.find_best_parameters(**kw)
    assert np.unravel_index(np.nanargmax(corr), corr.shape) != best
    F = A.find_local_shifts(**kw, tile_shape=(12, 10), method=MI, bins=bins, sub_lag=False)
    assert F.valid.all() and np.all(F.shift_dx == -2.0) and np.all(F.shift_dy == 3.0) and F.median_shift == (-2.0, 3.0)
    D = F.destretch(A.data_small)
    fin = np.isfinite(D)
    assert D.shape == A.data_small.shape and fin.sum() >= A.data_small.size - 20 and not fin[np.isnan(A.data_small)].any()
    assert np.array_equal(D[fin], A.data_small[fin])


# ------------------------------------------------------------------------------------------------------------- refusals
def _code(fn, *args, **kw):
    with pytest.raises(_lib.CoregError) as e:
        fn(*args, **kw)
    return e.value.code


def test_refusals_by_error_code(objects):
    A, kw = objects["c"]
    plan = A.host_plan(**kw, tile_shape=(10, 9))  # (no "bins": the handle's own lists are used)
    ok = np.arange(1.0, 32.0)
    with _lib.CoregHandle(0) as hnd:
        hnd.pixels_set_large(A.data_large)
        hnd.pixels_set_small(A.data_small)
        assert _code(hnd.pixels_sweep, plan, _lib.METHOD_MUTUAL_INFORMATION) == _lib.COREG_ESTATE  # no bins set
        assert _code(hnd.pixels_sweep_tiles, plan, _lib.METHOD_MUTUAL_INFORMATION) == _lib.COREG_ESTATE
        for bad in ([], np.arange(32.0), [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf], [-np.inf, 0.0]):
            assert _code(hnd.pixels_set_bins, bad, ok) == _lib.COREG_EINVAL
            assert _code(hnd.pixels_set_bins, ok, bad) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep, plan, _lib.METHOD_MUTUAL_INFORMATION) == _lib.COREG_ESTATE  # still none
        mi_plan = A.host_plan(**kw, method=MI, bins=8, tile_shape=(10, 9))
        hnd.pixels_set_bins(*mi_plan["bins"])
        cube = hnd.pixels_sweep(plan, _lib.METHOD_MUTUAL_INFORMATION)
        assert _code(hnd.pixels_set_bins, [2.0, 1.0], ok) == _lib.COREG_EINVAL
        # the lists stay until set again: after a refused call, another score and new images
        hnd.pixels_sweep(plan, _lib.METHOD_CORRELATION)
        hnd.pixels_set_small(A.data_small)
        assert np.array_equal(hnd.pixels_sweep(plan, _lib.METHOD_MUTUAL_INFORMATION), cube, equal_nan=True)
        assert np.array_equal(hnd.pixels_sweep(mi_plan, _lib.METHOD_MUTUAL_INFORMATION), cube, equal_nan=True)
        counts = hnd.pixels_last_counts(cube.shape)
        tiles = hnd.pixels_sweep_tiles(plan, _lib.METHOD_MUTUAL_INFORMATION)
        assert np.array_equal(hnd.pixels_last_tile_counts(tiles.shape).sum(axis=(0, 1)), counts)
        assert _code(hnd.pixels_last_counts, cube.shape) == _lib.COREG_ESTATE  # after a tiled sweep
        assert _code(hnd.pixels_sweep, plan, _lib.METHOD_RESIDUS) == _lib.COREG_ENOTIMPL
        assert _code(hnd.pixels_sweep_tiles, plan, _lib.METHOD_RESIDUS) == _lib.COREG_ENOTIMPL
        assert _code(hnd.pixels_sweep, plan, 7) == _lib.COREG_EINVAL
    assert np.array_equal(cube, A.find_best_parameters(**kw, method=MI, bins=8), equal_nan=True)
