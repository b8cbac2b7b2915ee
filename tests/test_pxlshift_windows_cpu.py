"""
CPU tests of the sliding, apodized windows of the local shift field (pxlshift `find_local_shifts(tile_step=...,
apodization=...)`): the window grid worked by hand, the weighted coefficient of the numpy
restatement tests/pxlshift_windows_oracle.py worked by hand, the arguments of `host_plan`, the two-drift scene on a
stepped grid, and `LocalShiftField` with a step.  No GPU.

The two-drift scene (tests/pxlshift_tiles_cases.py) in windows of (20, 24) at step (10, 12), a 3 x 3 grid: the six
windows whose columns lie in one half (column starts 0 and 24) give that half's lag at 0.99944 - 0.99974 against
runners-up of 0.588 - 0.757 unapodized and 0.606 - 0.718 with sigma = (5, 6) (printed; asserted: the lag and a lead of
0.1); the three windows that start at column 12 hold both halves and are not asserted.
"""
import numpy as np
import pytest

from euispice_coreg_amd.pxlshift import LocalShiftField
from euispice_coreg_amd.pxlshift.alignment_pixels import apodization_tables, gaussian_window, tile_grid, window_slices

from . import pxlshift_cases as Cs
from . import pxlshift_tiles_cases as TC
from . import pxlshift_tiles_oracle as T
from . import pxlshift_windows_oracle as Wd


# ------------------------------------------------------------------------------------------------------- the grid
def test_grid_rule_by_hand():
    assert Wd.axis_windows(10, 4, 2) == [(0, 4), (2, 6), (4, 8), (6, 10)]
    assert Wd.axis_windows(11, 4, 2) == [(0, 4), (2, 6), (4, 8), (6, 10), (8, 11)]  # a fifth, ragged window
    assert Wd.axis_windows(4, 4, 2) == [(0, 4)] and Wd.axis_windows(3, 4, 1) == [(0, 3)]  # h <= th: one window
    for h in range(1, 30):
        for th in range(1, h + 1):
            assert len(Wd.axis_windows(h, th, th)) == -(-h // th)  # sy = th: the disjoint tiles
            assert tile_grid((h, 7), (th, 3), (th, 3)) == tile_grid((h, 7), (th, 3)) == ((th, 3), (-(-h // th), 3))
            for sy in range(1, th + 1):
                wins = Wd.axis_windows(h, th, sy)
                assert wins[0][0] == 0 and wins[-1][1] == h
                covered = np.zeros(h, dtype=bool)
                for a, b in wins:
                    covered[a:b] = True
                assert covered.all()  # every pixel is covered
                assert all(b2 > b1 for (_, b1), (_, b2) in zip(wins, wins[1:]))  # no window inside its neighbour
                centres = [(a + b - 1) / 2 for a, b in wins]
                assert all(c2 > c1 for c1, c2 in zip(centres, centres[1:]))  # strictly increasing
                # the package's grid and slices are the oracle's
                assert tile_grid((h, 7), (th, 3), (sy, 2))[1] == (len(wins), 3)
                sl = window_slices((h, 7), (th, 3), (sy, 2))
                assert [(r.start, r.stop) for r in (row[0][0] for row in sl)] == wins
                assert [(c.start, c.stop) for _, c in sl[0]] == [(0, 3), (2, 5), (4, 7)]
    assert window_slices((25, 21), (10, 9)) == T.tile_slices((25, 21), (10, 9))
    assert Wd.window_slices((25, 21), (10, 9)) == T.tile_slices((25, 21), (10, 9))


def test_grid_refusals_and_plan(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    h, w = A.data_small.shape  # 25 x 21
    p = A.host_plan(**kw, tile_shape=(10, 9))
    assert p["tile_step"] == (10, 9) and p["tile_grid"] == (3, 3) and p["window"] is None
    p = A.host_plan(**kw, tile_shape=(10, 9), tile_step=(4, np.int64(5)))
    assert p["tile_shape"] == (10, 9) and p["tile_step"] == (4, 5) and p["tile_grid"] == (5, 4)
    assert all(type(v) is int for v in p["tile_step"] + p["tile_grid"])
    assert A.host_plan(**kw, tile_shape=(h, w), tile_step=(1, 1))["tile_grid"] == (1, 1)
    for bad in ((0, 5), (4, 0), (11, 5), (4, 10), (-1, 5), (2.0, 5), (True, 5), (5,), (5, 5, 5), 5, "ab"):
        with pytest.raises(ValueError):
            A.host_plan(**kw, tile_shape=(10, 9), tile_step=bad)
        with pytest.raises(ValueError):
            tile_grid((h, w), (10, 9), bad)
    with pytest.raises(ValueError):  # a step or an apodization without a tile shape
        A.host_plan(**kw, tile_step=(4, 5))
    with pytest.raises(ValueError):
        A.host_plan(**kw, apodization="gaussian")
    for method in ("correlation", "residus_masked", "mutual_information"):  # the grid belongs to every method
        assert A.host_plan(**kw, tile_shape=(10, 9), tile_step=(4, 5), method=method)["tile_grid"] == (5, 4)


# ---------------------------------------------------------------------------------------------------- the weights
def test_weighted_coefficient_by_hand():
    """A 2 x 2 window, weights 1, 2, 3, 4 (wy = (1, 3), wx = (1, 4 / 3) would not be exact: the weights are given): a =
    (1, 2, 3, 5), b = (2, 1, 4, 3).  W = 10, am = 34 / 10, bm = 28 / 10; da = (-2.4, -1.4, -0.4, 1.6), db = (-0.8, -1.8, 1.2,
    0.2); sum w da db = 6.8, sum w da^2 = 20.4, sum w db^2 = 11.6: corr = 6.8 / sqrt(20.4 * 11.6) = 0.44204..."""
    a = np.array([[1.0, 2.0], [3.0, 5.0]])
    b = np.array([[2.0, 1.0], [4.0, 3.0]])
    w = np.array([[1.0, 2.0], [3.0, 4.0]])
    corr, n, W = Wd.weighted(b, a, w)
    want = 6.8 / np.sqrt(20.4 * 11.6)
    assert n == 4 and W == 10.0 and abs(corr - want) <= 2.0 ** -23 * want + 1e-12 and abs(want - 0.44204) < 1e-5
    # tables: w = wy[r] * wx[c], a ragged window the head of the tables
    assert np.array_equal(Wd.weights_of([1.0, 3.0], [1.0, 2.0, 9.0], (2, 2)), [[1.0, 2.0], [3.0, 6.0]])
    # a zero-weight pixel counts in n, not in W, and does not move the score
    w0 = np.array([[1.0, 2.0], [3.0, 0.0]])
    c0, n0, W0 = Wd.weighted(b, a, w0)
    c3, n3, W3 = Wd.weighted(b.ravel()[:3], a.ravel()[:3], w0.ravel()[:3])
    assert (n0, W0, n3, W3) == (4, 6.0, 3, 6.0) and c0 == c3
    # a NaN pixel leaves n and W
    a2 = a.copy()
    a2[0, 1] = np.nan
    assert Wd.weighted(b, a2, w)[1:] == (3, 8.0)
    # NaN when W = 0 or a variance is 0
    r = Wd.weighted(b, a, np.zeros((2, 2)))
    assert np.isnan(r[0]) and r[1:] == (4, 0.0)
    assert np.isnan(Wd.weighted(b, np.full((2, 2), 3.0), w)[0]) and np.isnan(Wd.weighted(np.full((2, 2), 3.0), a, w)[0])
    one = np.array([[0.0, 0.0], [0.0, 2.0]])  # one weighted pixel: both variances 0
    assert np.isnan(Wd.weighted(b, a, one)[0])
    r = Wd.weighted(np.full((2, 2), np.nan), a, w)
    assert np.isnan(r[0]) and r[1:] == (0, 0.0)


def test_tables_of_ones_are_the_unweighted_coefficient(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    plan = A.host_plan(**kw, tile_shape=(10, 9), tile_step=(4, 5))
    ones = (np.ones(10), np.ones(9))
    o = Wd.scores(A.data_large, A.data_small, plan, (10, 9), (4, 5), window=ones)
    assert o["corr"].shape == (5, 4, 7, 5, 3) and np.isfinite(o["corr"]).all()
    assert np.array_equal(o["wcorr"], o["corr"])  # pxlshift_oracle.correlate, to the bit
    assert np.array_equal(o["weight"], o["count"])
    # and a window that coincides with a disjoint tile holds that tile's figures: step (5, 9) on 25 rows gives the
    # windows [0, 10), [5, 15), [10, 20), [15, 25) -- windows 0 and 2 are tiles 0 and 1 (the ragged tile [20, 25) lies
    # inside the last window, so the grid rule gives it no window of its own)
    t = T.scores(A.data_large, A.data_small, plan, (10, 9))
    s = Wd.scores(A.data_large, A.data_small, plan, (10, 9), (5, 9))
    assert s["corr"].shape[:2] == (4, 3)
    for key in T.KEYS:
        assert np.array_equal(s[key][[0, 2]], t[key][[0, 1]], equal_nan=True)


def test_gaussian_tables_and_refusals(tmp_path):
    for n, sigma in ((10, 2.5), (9, 2.25), (1, 0.25), (64, 16.0)):
        r = np.arange(n)
        want = np.exp(-0.5 * ((r - (n - 1) / 2) / sigma) ** 2)
        assert np.array_equal(gaussian_window(n, sigma), want) and np.array_equal(Wd.gaussian_table(n, sigma), want)
        assert np.array_equal(want, want[::-1]) and want.max() <= 1.0 and want.dtype == np.float64
    wy, wx = apodization_tables("gaussian", (10, 9))
    assert np.array_equal(wy, gaussian_window(10, 2.5)) and np.array_equal(wx, gaussian_window(9, 2.25))
    wy, wx = apodization_tables((5.0, 6), (20, 24))
    assert np.array_equal(wy, gaussian_window(20, 5.0)) and np.array_equal(wx, gaussian_window(24, 6.0))
    ty, tx = np.linspace(0.0, 1.0, 10), np.ones(9, dtype=np.float32)
    wy, wx = apodization_tables((ty, tx), (10, 9))
    assert np.array_equal(wy, ty) and np.array_equal(wx, np.ones(9)) and wx.dtype == np.float64 and wy is not ty
    assert apodization_tables(None, (10, 9)) is None
    neg, nan, zero = np.ones(10), np.ones(10), np.zeros(10)
    neg[3], nan[4] = -0.1, np.nan
    A, kw = Cs.make("a", tmp_path)
    for bad in ("hann", 3.0, (2.0,), (2.0, 0.0), (-1.0, 2.0), (np.inf, 2.0), (np.nan, 2.0), (True, 2.0), (2.0, 2.0, 2.0),
                (np.ones(9), np.ones(9)), (np.ones(10), np.ones(10)), (np.ones((10, 1)), np.ones(9)), (neg, np.ones(9)),
                (nan, np.ones(9)), (zero, np.ones(9)), (np.ones(10), np.zeros(9)), (np.ones(10), 2.0),
                (np.full(10, np.inf), np.ones(9))):
        with pytest.raises(ValueError):
            apodization_tables(bad, (10, 9))
        with pytest.raises(ValueError):
            A.host_plan(**kw, tile_shape=(10, 9), apodization=bad)
    p = A.host_plan(**kw, tile_shape=(10, 9), tile_step=(4, 5), apodization="gaussian")
    assert np.array_equal(p["window"][0], gaussian_window(10, 2.5)) and np.array_equal(p["window"][1], gaussian_window(9, 2.25))
    for method in ("residus_masked", "mutual_information"):  # no weighted residus_masked, no weighted histogram
        with pytest.raises(ValueError, match="apodization"):
            A.host_plan(**kw, tile_shape=(10, 9), apodization="gaussian", method=method)
        with pytest.raises(ValueError, match="apodization"):  # (refused before any GPU work)
            A.find_local_shifts(kw["lag_dx"], kw["lag_dy"], tile_shape=(10, 9), apodization=(2.0, 2.0), method=method)


# ------------------------------------------------------------------------------------------------ two-drift scene
STEP, SIGMA = (10, 12), (5.0, 6.0)


@pytest.fixture(scope="module")
def two_drift():
    A, kw, tile_shape, want = TC.two_drift_object()
    plan = A.host_plan(**kw, tile_shape=tile_shape, tile_step=STEP, apodization=SIGMA)
    o = Wd.scores(A.data_large, A.data_small, plan, tile_shape, STEP, window=plan["window"])
    return A, kw, plan, want, o


def test_two_drift_scene_on_a_stepped_grid(two_drift):
    A, kw, plan, want, o = two_drift
    assert plan["tile_shape"] == (20, 24) and plan["tile_grid"] == (3, 3) and o["corr"].shape == (3, 3, 9, 9, 1)
    lag = kw["lag_dx"]
    for key in ("corr", "wcorr"):
        for ty in range(3):
            for tx, half in ((0, want[0][0]), (2, want[0][1])):  # column starts 0 and 24: one half each
                c = o[key][ty, tx, :, :, 0]
                b = np.unravel_index(np.nanargmax(c), c.shape)
                top = np.sort(c.ravel())[-2:]
                print(key, (ty, tx), "best", lag[b[0]], lag[b[1]], "top two", top[1], top[0])
                assert (lag[b[0]], lag[b[1]]) == half
                assert top[1] - top[0] >= 0.1
    assert half == (-1, 2) and want[0][0] == (2, -1)
    assert np.array_equal(o["count"][0, 0], T.scores(A.data_large, A.data_small, plan, (20, 24))["count"][0, 0])
    assert np.all(o["weight"] < o["count"]) and np.all(o["weight"] > 0)
    for wcube, F in ((None, None), (o["weight"], plan["window"])):
        F = LocalShiftField(o["corr" if F is None else "wcorr"], o["count"], plan["lag_dx"], plan["lag_dy"], plan["lag_drot"],
                            plan["tile_shape"], A.data_small.shape, tile_step=STEP, weight_sums=wcube, window=F)
        assert F.valid.all() and F.shift_dx.shape == (3, 3)
        for tx, (dx, dy) in ((0, want[0][0]), (2, want[0][1])):
            assert np.all(np.abs(F.shift_dx[:, tx] - dx) < 0.1) and np.all(np.abs(F.shift_dy[:, tx] - dy) < 0.1)
        D = F.drift()
        assert D[0, 1] < -0.05 and D[1, 1] > 0.05  # dx falls, dy rises across the raster


# ------------------------------------------------------------------------------------- LocalShiftField with a step
def _peaks(grid, n_lag=11):
    corr = np.full(grid + (n_lag, n_lag, 1), 0.1)
    dx, dy = np.zeros(grid, dtype=int), np.zeros(grid, dtype=int)
    for ty in range(grid[0]):
        for tx in range(grid[1]):
            dx[ty, tx], dy[ty, tx] = tx - 2, 1 - ty
            corr[ty, tx, dx[ty, tx] + 5, dy[ty, tx] + 5, 0] = 0.9
    return corr, dx, dy


def test_field_with_a_step():
    lag = np.arange(-5, 6)
    shape, tile, step = (30, 42), (10, 12), (10, 6)  # rows disjoint (3), columns half-overlapping: ceil(30 / 6) + 1 = 6
    corr, dx, dy = _peaks((3, 6))
    counts = np.full(corr.shape, 100.0)
    F = LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, sub_lag=False, tile_step=step)
    assert F.tile_shape == tile and F.tile_step == step and F.weight_sums is None and F.window is None
    assert [c for _, c in F.tile_slices[0]] == [slice(6 * k, 6 * k + 12) for k in range(6)]
    assert [row[0][0] for row in F.tile_slices] == [slice(0, 10), slice(10, 20), slice(20, 30)]
    assert F.tile_centres[0, :, 0].tolist() == [5.5, 11.5, 17.5, 23.5, 29.5, 35.5] and F.tile_centres[:, 0, 1].tolist() == \
        [4.5, 14.5, 24.5]
    assert np.array_equal(F.shift_dx, dx) and np.array_equal(F.shift_dy, dy) and F.valid.all()
    D = F.drift()  # dx = tx - 2 = (xc - 5.5) / 6 - 2, dy = 1 - ty = 1 - (yc - 4.5) / 10
    assert np.allclose(D, [[-2 - 5.5 / 6, 1 / 6, 0.0], [1.45, 0.0, -0.1]], rtol=0, atol=1e-12)
    u, v = F.node_shifts(reference=(0.0, 0.0))
    assert np.array_equal(u, dx) and np.array_equal(v, dy)
    assert F.median_shift == (0.5, 0.0)
    # a ragged last window: 43 columns give a seventh window [36, 43), its centre that of the clipped rectangle
    corr7, _, _ = _peaks((3, 7))
    G = LocalShiftField(corr7, np.full(corr7.shape, 100.0), lag, lag, [0.0], tile, (30, 43), sub_lag=False, tile_step=step)
    assert G.tile_slices[0][6][1] == slice(36, 43) and G.tile_centres[0, 6, 0] == 39.0
    # the shape check uses the stepped grid
    with pytest.raises(ValueError):
        LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, sub_lag=False)  # (3, 4) without the step
    with pytest.raises(ValueError):
        LocalShiftField(corr7, np.full(corr7.shape, 100.0), lag, lag, [0.0], tile, shape, sub_lag=False, tile_step=step)
    with pytest.raises(ValueError):
        LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, tile_step=(11, 6))
    # "the value of the pixel's tile" has no meaning for overlapping windows (refused before any GPU work)
    with pytest.raises(ValueError, match="nearest"):
        F.destretch(np.zeros(shape), interpolation="nearest")
    # the step given as the tile shape is the disjoint field
    c4, _, _ = _peaks((3, 4))
    H = LocalShiftField(c4, np.full(c4.shape, 100.0), lag, lag, [0.0], tile, shape, sub_lag=False, tile_step=tile)
    K = LocalShiftField(c4, np.full(c4.shape, 100.0), lag, lag, [0.0], tile, shape, sub_lag=False)
    assert H.tile_slices == K.tile_slices and H.tile_step == K.tile_step == tile
    assert np.array_equal(H.tile_centres, K.tile_centres)


def test_field_min_fill_compares_weights():
    """A window of 10 x 12 under sigma = (2.5, 3): the sum of its weights is 43.04 of 120 pixels.  A window whose kept
    pixels are its corners holds half the pixels and little of the weight."""
    lag = np.arange(-5, 6)
    shape, tile, step = (10, 30), (10, 12), (10, 6)
    corr, dx, dy = _peaks((1, 4))
    wy, wx = gaussian_window(10, 2.5), gaussian_window(12, 3.0)
    full = np.outer(wy, wx).sum()
    counts = np.full(corr.shape, 70.0)
    weights = np.full(corr.shape, 0.9 * full)
    weights[0, 1] = 0.2 * full  # 70 of 120 pixels kept, a fifth of the weight
    kw = dict(sub_lag=False, tile_step=step)
    F = LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, weight_sums=weights, window=(wy, wx), **kw)
    assert F.valid.tolist() == [[True, False, True, True]] and np.array_equal(F.weight_sums, weights)
    assert np.array_equal(F.n_samples, counts)
    assert LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, **kw).valid.all()  # by pixels it would pass
    with pytest.raises(ValueError):  # no valid window at all
        LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, weight_sums=weights, window=(wy, wx), min_fill=0.95, **kw)
    # a ragged window is measured against the head of the tables: 28 columns leave [18, 28), 10 of 12 columns
    head = np.outer(wy, wx[:10]).sum()
    w2 = np.full(corr.shape, 0.9 * full)
    w2[0, 3] = 0.52 * head
    R = LocalShiftField(corr, counts, lag, lag, [0.0], tile, (10, 28), weight_sums=w2, window=(wy, wx), min_fill=0.5, **kw)
    assert R.tile_slices[0][3][1] == slice(18, 28) and R.valid.all() and 0.5 * head < 0.52 * head < 0.5 * full
    for bad in (dict(weight_sums=weights), dict(window=(wy, wx)), dict(weight_sums=weights[:, :2], window=(wy, wx)),
                dict(weight_sums=weights, window=(wy, wx[:10])),
                dict(weight_sums=weights, window=(wy, wx), method="residus_masked")):
        with pytest.raises(ValueError):
            LocalShiftField(corr, counts, lag, lag, [0.0], tile, shape, **kw, **bad)
