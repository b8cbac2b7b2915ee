"""
CPU tests of the local shift field of the pixel-lag alignment (pxlshift): the numpy restatement
tests/pxlshift_tiles_oracle.py against figures computed independently from the definitions and against the untiled
oracle, the tile grid of `host_plan`, `LocalShiftField` on oracle cubes, and the two-drift scene.  No GPU.

The two-drift scene (tests/pxlshift_tiles_cases.py): on the object's own prepared images -- the order-1 sub-resolution at
ratio 1 spreads every NaN of the large image to the taps of weight 0 next to it, which the figures of the raw images
(counts 467 - 474, global best 0.516) do not have -- the tiles' bests are (2, -1) left and (-1, 2) right at 0.9994 - 0.9997
against runners-up of at most 0.690, counts 452 - 471 per tile and lag, and the best single lag of the whole image scores
0.509.
"""
import numpy as np
import pytest

from euispice_coreg_amd.pxlshift import LocalShiftField

from . import pxlshift_cases as Cs
from . import pxlshift_oracle as O
from . import pxlshift_scores_oracle as S
from . import pxlshift_tiles_cases as TC
from . import pxlshift_tiles_oracle as T


@pytest.fixture(scope="module")
def case_a(tmp_path_factory):
    """Case a in tiles of (10, 9) -- 3 x 3 tiles of a 25 x 21 image, ragged on both axes: (object, kw, plan, cubes)."""
    A, kw = Cs.make("a", tmp_path_factory.mktemp("pxt_a"))
    plan = A.host_plan(**kw, tile_shape=(10, 9))
    return A, kw, plan, T.scores(A.data_large, A.data_small, plan, plan["tile_shape"])


@pytest.fixture(scope="module")
def two_drift():
    A, kw, tile_shape, want = TC.two_drift_object()
    plan = A.host_plan(**kw, tile_shape=tile_shape)
    return A, kw, plan, want, T.scores(A.data_large, A.data_small, plan, tile_shape)


def test_figures_of_case_a_from_the_definitions(case_a):
    """np.corrcoef and a mean-of-squares standard deviation on the rectangle cut by hand, three (tile, lag) pairs: a
    ragged corner tile of 5 x 3 pixels, the first tile, the middle tile at a rotated plane."""
    A, kw, plan, o = case_a
    assert A.data_small.shape == (25, 21) and o["corr"].shape == (3, 3, 7, 5, 3)
    sub = O.sub_resolution(A.data_large, plan["ratio_res_1"], plan["ratio_res_2"])
    l = plan["slc_small_ref"]
    for (ty, tx, i, j, k), n in (((2, 2, 4, 1, 1), 12), ((0, 0, 0, 0, 0), 86), ((1, 1, 4, 1, 1), 80)):
        dx, dy = int(kw["lag_dx"][i]), int(kw["lag_dy"][j])
        win = sub[l[0] + dy:l[0] + dy + 25, l[1] + dx:l[1] + dx + 21][10 * ty:10 * ty + 10, 9 * tx:9 * tx + 9]
        plane = O.rotate(A.data_small, kw["lag_drot"][k], kw["unit_rot"])[10 * ty:10 * ty + 10, 9 * tx:9 * tx + 9]
        x, y = win.ravel(), plane.ravel()
        m = np.isfinite(x) & np.isfinite(y)
        d = (x[m] - y[m]) / np.sqrt(x[m])
        want_corr, want_std = np.corrcoef(x[m], y[m])[0, 1], np.sqrt(np.mean((d - d.mean()) ** 2))
        got = {key: o[key][ty, tx, i, j, k] for key in T.KEYS}
        print((ty, tx, i, j, k), "n", m.sum(), "corr", got["corr"], want_corr, "masked", got["masked"], want_std)
        assert m.sum() == n == got["count"] == got["finite_terms"] and got["poisoned"] == 0
        assert abs(got["corr"] - want_corr) <= 2.0 ** -23 * abs(want_corr) + 1e-12  # (the float32 numerator)
        assert abs(got["masked"] - want_std) <= 1e-14 * want_std
    assert o["count"].max(axis=(2, 3, 4)).tolist() == [[87, 89, 30], [88, 87, 28], [43, 45, 15]]
    assert o["count"].min(axis=(2, 3, 4)).tolist() == [[58, 72, 14], [75, 80, 17], [32, 38, 8]]
    assert [round(float(o["corr"][t]), 6) for t in ((2, 2, 4, 1, 1), (0, 0, 0, 0, 0), (1, 1, 4, 1, 1))] == \
        [0.735921, 0.733988, 0.638130]


@pytest.mark.parametrize("name,tile_shape", [("a", (10, 9)), ("b", (40, 50)), ("c", (10, 9))])
def test_oracle_against_the_untiled_oracle(name, tile_shape, tmp_path):
    A, kw = Cs.make(name, tmp_path)
    plan = A.host_plan(**kw)
    u = S.scores(A.data_large, A.data_small, plan)
    o = T.scores(A.data_large, A.data_small, plan, tile_shape)
    h, w = A.data_small.shape
    assert o["corr"].shape[:2] == (-(-h // tile_shape[0]), -(-w // tile_shape[1])) and h % tile_shape[0] and w % tile_shape[1]
    for key in ("count", "finite_terms", "poisoned"):  # whole numbers: the tiles' sum is the image's, exactly
        assert np.array_equal(o[key].sum(axis=(0, 1)), u[key])
    one = T.scores(A.data_large, A.data_small, plan, (h, w))
    for key in T.KEYS:
        assert one[key].shape == (1, 1) + u[key].shape and np.array_equal(one[key][0, 0], u[key], equal_nan=True)


def test_tile_grid_of_host_plan(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    h, w = A.data_small.shape
    assert "tile_shape" not in A.host_plan(**kw)
    for shape, grid in (((10, 9), (3, 3)), ((h, w), (1, 1)), ((h, 1), (1, w)), ((1, w), (h, 1)), ((13, 11), (2, 2)),
                        ((5, 7), (5, 3)), ((np.int64(12), 20), (3, 2))):
        p = A.host_plan(**kw, tile_shape=shape)
        assert p["tile_shape"] == tuple(shape) and p["tile_grid"] == grid and p["small_shape"] == (h, w)
        assert all(type(v) is int for v in p["tile_shape"] + p["tile_grid"])
        sl = T.tile_slices((h, w), p["tile_shape"])
        assert (len(sl), len(sl[0])) == grid
        assert sl[-1][-1][0].stop == h and sl[-1][-1][1].stop == w  # the last tile ends with the image, ragged or not
    for bad in ((0, 5), (5, 0), (h + 1, 5), (5, w + 1), (-1, 5), (2.0, 5), (True, 5), (5,), (5, 5, 5), 5, "ab"):
        with pytest.raises(ValueError):
            A.host_plan(**kw, tile_shape=bad)
    with pytest.raises(ValueError):  # find_local_shifts needs a shape (refused before any GPU work)
        A.find_local_shifts(kw["lag_dx"], kw["lag_dy"])
    with pytest.raises(NotImplementedError):
        A.host_plan(**kw, tile_shape=(10, 9), method="residus")


# ----------------------------------------------------------------------------------------------- LocalShiftField
def _field(case, key="corr", counts="count", **kw):
    A, ckw, plan, o = case[0], case[1], case[2], case[-1]
    return LocalShiftField(o[key], o[counts], plan["lag_dx"], plan["lag_dy"], plan["lag_drot"], plan["tile_shape"],
                           A.data_small.shape, unit_rot=plan["unit_rot"], **kw)


def test_field_valid_min_fill_and_min_overlap(case_a):
    A, kw, plan, o = case_a
    F = _field(case_a, sub_lag=False)
    assert F.corr.shape == F.n_samples.shape == (3, 3, 7, 5, 3) and F.valid.all()  # every tile holds half its pixels
    assert np.array_equal(F.corr, o["corr"], equal_nan=True) and np.array_equal(F.n_samples, o["count"])
    assert F.tile_slices[2][2] == (slice(20, 25), slice(18, 21)) and F.tile_slices[0][1] == (slice(0, 10), slice(9, 18))
    assert F.tile_centres.shape == (3, 3, 2)
    assert F.tile_centres[0, 0].tolist() == [4.0, 4.5] and F.tile_centres[2, 2].tolist() == [19.0, 22.0]  # (x, y)
    for ty in range(3):
        for tx in range(3):
            mi = np.unravel_index(np.nanargmax(o["corr"][ty, tx]), (7, 5, 3))
            assert tuple(F.best_index[ty, tx]) == mi and F.best_score[ty, tx] == o["corr"][ty, tx][mi]
            assert F.shift_dx[ty, tx] == kw["lag_dx"][mi[0]] and F.shift_dy[ty, tx] == kw["lag_dy"][mi[1]]
            assert F.drot[ty, tx] == kw["lag_drot"][mi[2]]
    assert F.best_index[..., 0].tolist() == [[4] * 3] * 3 and F.best_index[..., 1].tolist() == [[1] * 3] * 3
    assert not F.fitted.any() and "9 valid of 9 tiles" in str(F)
    # min_fill against the largest count over the pixel count of the tile itself: tile (0, 0) 87 / 90, tile (0, 2) 30 / 30,
    # tile (2, 1) 45 / 45, tile (1, 1) 87 / 90
    full = o["count"].max(axis=(2, 3, 4)) / np.array([[90, 90, 30], [90, 90, 30], [45, 45, 15]])
    G = _field(case_a, sub_lag=False, min_fill=0.97)
    assert np.array_equal(G.valid, full >= 0.97) and 0 < G.valid.sum() < 9
    bad = ~G.valid
    assert np.isnan(G.shift_dx[bad]).all() and np.isnan(G.shift_dy[bad]).all() and np.isnan(G.best_score[bad]).all()
    assert np.isnan(G.drot[bad]).all() and (G.best_index[bad] == -1).all() and (G.best_index[G.valid] >= 0).all()
    assert np.array_equal(G.corr, F.corr, equal_nan=True)  # (min_fill hides no entry)
    # min_overlap per tile: a fraction of the tile's own largest count, and a count
    H = _field(case_a, sub_lag=False, min_overlap=0.9)
    for ty in range(3):
        for tx in range(3):
            c = o["count"][ty, tx]
            assert np.array_equal(np.isnan(H.corr[ty, tx]), c < 0.9 * c.max())
    assert np.array_equal(H.n_samples, o["count"]) and H.valid.all()
    K = _field(case_a, sub_lag=False, min_overlap=46)  # more than any entry of the last row of tiles holds
    assert np.array_equal(np.isnan(K.corr), o["count"] < 46)
    assert K.valid.tolist() == [[True, True, False], [True, True, False], [False, False, False]]
    with pytest.raises(ValueError):  # no valid tile at all
        _field(case_a, sub_lag=False, min_overlap=100)
    for bad_mo in (0, 1.5, True):
        with pytest.raises(ValueError):
            _field(case_a, min_overlap=bad_mo)
    with pytest.raises(ValueError):
        _field(case_a, min_fill=1.5)
    with pytest.raises(NotImplementedError):
        _field(case_a, method="residus")
    with pytest.raises(ValueError):
        LocalShiftField(o["corr"][:2], o["count"][:2], plan["lag_dx"], plan["lag_dy"], plan["lag_drot"], (10, 9), (25, 21))


def test_field_minimum_of_residus_masked(case_a):
    A, kw, plan, o = case_a
    F = _field(case_a, "masked", "finite_terms", method="residus_masked", sub_lag=False)
    assert F.best == "min" and F.valid.all()
    for ty in range(3):
        for tx in range(3):
            mi = np.unravel_index(np.nanargmin(o["masked"][ty, tx]), (7, 5, 3))
            assert tuple(F.best_index[ty, tx]) == mi and F.best_score[ty, tx] == o["masked"][ty, tx].min()


def test_field_statistics_and_drift():
    """Cubes with one peak per tile at a lag that is a plane of the tile centre: the medians, the scatter and the drift are
    known in closed form."""
    lag = np.arange(-5, 6)
    shape, tile = (30, 40), (10, 10)  # 3 x 4 tiles, centres x = 4.5, 14.5, 24.5, 34.5, y = 4.5, 14.5, 24.5
    corr = np.full((3, 4, 11, 11, 1), 0.1)
    want_dx, want_dy = np.zeros((3, 4), dtype=int), np.zeros((3, 4), dtype=int)
    for ty in range(3):
        for tx in range(4):
            want_dx[ty, tx], want_dy[ty, tx] = tx - 1, 1 - ty  # dx = -1.45 + 0.1 xc, dy = 1.45 - 0.1 yc
            corr[ty, tx, want_dx[ty, tx] + 5, want_dy[ty, tx] + 5, 0] = 0.9
    counts = np.full(corr.shape, 100.0)
    F = LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, sub_lag=False)
    assert np.array_equal(F.shift_dx, want_dx) and np.array_equal(F.shift_dy, want_dy) and F.valid.all()
    assert F.median_shift == (0.5, 0.0)
    assert F.scatter == (1.4826 * 1.0, 1.4826 * 1.0)  # |dx - 0.5| = 1.5, 0.5, 0.5, 1.5 per row; |dy| = 1, 0, 1 per column
    D = F.drift()
    assert D.shape == (2, 3) and np.allclose(D, [[-1.45, 0.1, 0.0], [1.45, 0.0, -0.1]], rtol=0, atol=1e-12)
    # invalid tiles do not vote: empty the last column of tiles
    counts2 = counts.copy()
    counts2[:, 3] = 10.0
    G = LocalShiftField(corr, counts2, lag, lag, [0.0], tile, shape, sub_lag=False)
    assert G.valid.sum() == 9 and not G.valid[:, 3].any() and G.median_shift == (0.0, 0.0)
    assert np.allclose(G.drift(), D, rtol=0, atol=1e-12)
    # fewer than three valid tiles, and three collinear ones
    counts3 = np.full(corr.shape, 10.0)
    counts3[0, :2] = 100.0
    with pytest.raises(ValueError, match="three valid"):
        LocalShiftField(corr, counts3, lag, lag, [0.0], tile, shape, sub_lag=False).drift()
    counts3[0, 2] = 100.0
    L = LocalShiftField(corr, counts3, lag, lag, [0.0], tile, shape, sub_lag=False)
    assert L.valid.sum() == 3 and np.isfinite(L.median_shift).all() and np.isfinite(L.scatter).all()
    with pytest.raises(ValueError, match="collinear"):
        L.drift()


def test_field_sub_lag_fit_is_the_fit_of_the_results_object():
    from euispice_coreg_amd.pxlshift import PixelAlignmentResults
    x, y = np.meshgrid(np.arange(9.0), np.arange(7.0), indexing="ij")
    peaks = [(4.3, 2.6), (3.7, 3.2)]
    cubes = [np.stack([0.5 * g, g], axis=2) for g in
             (0.8 * np.exp(-((x - px) ** 2 / 4.0 + (y - py) ** 2 / 3.0)) for px, py in peaks)]
    corr = np.stack(cubes)[None]  # one row of two tiles
    lag_dx, lag_dy, lag_drot = np.arange(-4, 5), np.arange(-6, 8, 2), np.array([-0.5, 0.5])
    F = LocalShiftField(corr, np.full(corr.shape, 50.0), lag_dx, lag_dy, lag_drot, (5, 10), (5, 20))
    assert F.fitted.all() and F.valid.all()
    for tx, cube in enumerate(cubes):
        R = PixelAlignmentResults(cube, lag_dx, lag_dy, lag_drot)
        assert (F.shift_dx[0, tx], F.shift_dy[0, tx]) == R.shift_pixels and F.drot[0, tx] == R.drot == 0.5
        assert tuple(F.best_index[0, tx]) == R.max_index
    assert abs(F.shift_dx[0, 0] - 0.3) < 1e-6 and abs(F.shift_dx[0, 1] + 0.3) < 1e-6
    N = LocalShiftField(corr, np.full(corr.shape, 50.0), lag_dx, lag_dy, lag_drot, (5, 10), (5, 20), sub_lag=False)
    assert not N.fitted.any() and N.shift_dx.tolist() == [[0.0, 0.0]] and N.shift_dy.tolist() == [[0.0, 0.0]]


# ------------------------------------------------------------------------------------------------ two-drift scene
def test_two_drift_scene(two_drift):
    A, kw, plan, want, o = two_drift
    assert A.data_small.shape == (40, 48) and A.data_large.shape == (70, 86) and plan["tile_grid"] == (2, 2)
    assert (plan["ratio_res_1"], plan["ratio_res_2"]) == (1.0, 1.0) and tuple(plan["slc_small_ref"]) == (14, 18)
    assert np.isnan(A.data_small).sum() == 25 and 38 <= np.isnan(A.data_large).sum() <= 40
    u = S.scores(A.data_large, A.data_small, A.host_plan(**kw))
    lag = kw["lag_dx"]
    for ty in range(2):
        for tx in range(2):
            c = o["corr"][ty, tx, :, :, 0]
            b = np.unravel_index(np.nanargmax(c), c.shape)
            top = np.sort(c.ravel())[-2:]
            print((ty, tx), "best", lag[b[0]], lag[b[1]], "top two", top[1], top[0], "counts",
                  o["count"][ty, tx].min(), o["count"][ty, tx].max())
            assert (lag[b[0]], lag[b[1]]) == want[ty][tx]
            assert top[1] - top[0] > 0.3 and top[1] > 0.999
            m = o["masked"][ty, tx, :, :, 0]
            b = np.unravel_index(np.nanargmin(m), m.shape)
            assert (lag[b[0]], lag[b[1]]) == want[ty][tx]
    assert np.array_equal(o["count"].sum(axis=(0, 1)), u["count"])
    assert np.array_equal(o["finite_terms"].sum(axis=(0, 1)), u["finite_terms"])
    assert (o["count"].min(), o["count"].max()) == (452, 471)
    print("global best", np.nanmax(u["corr"]))
    assert round(float(np.nanmax(u["corr"])), 3) == 0.509  # no single lag fits the image
    F = _field((A, kw, plan, o))
    assert F.valid.all() and F.fitted.all()
    want = np.array(want)
    assert np.all(np.abs(F.shift_dx - want[..., 0]) < 0.1) and np.all(np.abs(F.shift_dy - want[..., 1]) < 0.1)
    assert F.median_shift == (float(np.median(F.shift_dx)), float(np.median(F.shift_dy)))
    assert 1.4826 * 1.4 < F.scatter[0] < 1.4826 * 1.6 and 1.4826 * 1.4 < F.scatter[1] < 1.4826 * 1.6  # halves 3 apart
    D = F.drift()
    assert D.shape == (2, 3) and abs(D[0, 1] + 3 / 24) < 0.01 and abs(D[1, 1] - 3 / 24) < 0.01 and np.all(np.abs(D[:, 2]) < 0.01)
