"""
GPU tests of the sliding, apodized windows of the local shift field (`AlignmentPixels.find_local_shifts(tile_step=...,
apodization=...)`, coreg_pixels_sweep_windows, k_pixels_lct of csrc/kernels_pixels_lct.hpp) against
tests/pxlshift_windows_oracle.py run on the object's own prepared planes and box (`A._rotated(k)`, `A._large_box()`).

Bounds, those of tests/test_gpu_pxlshift_tiles.py and tests/test_gpu_pxlshift_mi.py: counts are compared exactly; the
Pearson coefficient, weighted or not, within 2^-23 |corr| + 1e-12 (its numerator is rounded to float32); `residus_masked`
within 1e-10 relative; mutual information within 1e-11 absolute; the sums of weights within 1e-12 relative; the same NaN
pattern and the same best entry per window.  A step equal to the tile shape, a window that coincides with a disjoint
tile, a cube cut into several calls and the windows away from a changed one are compared bit for bit.

The shapes are the smallest that walk each path: ragged last windows on both axes at a step that divides neither the
image nor the tile, three rotation planes, ragged dx groups, a window of two column bands and one of two row bands
(csrc/kernels_pixels.hpp: a band is at most 2048 pixels and 64 rows, its shape that of the nominal tile).
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels, LocalShiftField

from . import pxlshift_cases as Cs
from . import pxlshift_destretch_oracle as D
from . import pxlshift_tiles_cases as TC
from . import pxlshift_windows_oracle as Wd

pytestmark = pytest.mark.gpu

MI = "mutual_information"
METHODS = ("correlation", "residus_masked", MI)
KEYS = {"correlation": ("corr", "count"), "residus_masked": ("masked", "finite_terms"), MI: ("mi", "mi_count")}
CASES = {"a": ((10, 9), (4, 5)), "c": ((10, 9), (4, 5)), "b": ((40, 50), (16, 32))}  # 25 x 21, 25 x 21, 70 x 130 pixels
GRIDS = {"a": (5, 4), "c": (5, 4), "b": (3, 4)}
BAND = 2048
worst = {}


def _local(A, kw, tile_shape, method="correlation", **more):
    """The raw cubes of a call: (corr, n_samples, field)."""
    F = A.find_local_shifts(**kw, tile_shape=tile_shape, method=method, sub_lag=False, min_fill=0.0, **more)
    assert isinstance(F, LocalShiftField) and F.corr.dtype == F.n_samples.dtype == np.float64
    return F.corr, F.n_samples, F


def _bound(want, method):
    if method == "correlation":
        return 2.0 ** -23 * np.abs(want) + 1e-12
    return 1e-10 * np.abs(want) if method == "residus_masked" else np.full(want.shape, 1e-11)


def _check(got, want, method, label, ties=False):
    """Every window's cube against the oracle's: the bound of the method, the NaN pattern, the best entry per window.
    ties (the rule of tests/test_gpu_pxlshift_tiles.py): another best entry passes when the oracle's own scores of the two
    lie within twice the bound."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), label
    fin = np.isfinite(want)
    d = np.abs(got[fin] - want[fin])
    bound = _bound(want, method)
    with np.errstate(all="ignore"):
        rel = d / np.abs(want[fin])
    m = (float(d.max()), float(np.nanmax(rel))) if d.size else (0.0, 0.0)
    worst[method] = tuple(max(a, b) for a, b in zip(worst.get(method, (0.0, 0.0)), m))
    print(label, method, "max |diff|", m[0], "max relative", m[1], "largest so far", worst[method])
    assert np.all(d <= bound[fin]), label
    arg = np.nanargmin if method == "residus_masked" else np.nanargmax
    for ty in range(want.shape[0]):
        for tx in range(want.shape[1]):
            if np.isfinite(want[ty, tx]).any():
                g, w = arg(got[ty, tx]), arg(want[ty, tx])
                if ties and g != w:
                    wt = want[ty, tx].ravel()
                    assert abs(wt[g] - wt[w]) <= 2 * bound[ty, tx].ravel()[w], (label, ty, tx)
                else:
                    assert g == w, (label, ty, tx)


def _check_weights(got, want, label):
    assert got.shape == want.shape and np.isfinite(got).all()
    with np.errstate(all="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / want, np.abs(got - want))
    worst["weights"] = max(worst.get("weights", 0.0), float(rel.max()))
    print(label, "weight sums: max relative", float(rel.max()), "largest so far", worst["weights"])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), label


def _oracle(A, kw, tile_shape, tile_step, apodization="gaussian", mi=True):
    """The oracle's cubes on the device's own planes and box of the last call of `A` with `kw`."""
    plan = A.host_plan(**kw, tile_shape=tile_shape, tile_step=tile_step, apodization=apodization)
    if mi:
        plan["bins"] = A.host_plan(**kw, method=MI)["bins"]
    planes, box = [A._rotated(k) for k in range(len(plan["lag_drot"]))], A._large_box()
    return plan, Wd.scores(None, A.data_small, plan, tile_shape, tile_step, window=plan["window"], planes=planes, box=box,
                           mi=mi)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Cases a, c, b once: object, arguments, plan, the oracle, per method the stepped (cube, counts), and the apodized
    field."""
    out = {}
    for name, (ts, step) in CASES.items():
        A, kw = Cs.make(name, tmp_path_factory.mktemp("pxw_" + name))
        per = {m: _local(A, kw, ts, m, tile_step=step)[:2] for m in METHODS}
        F = _local(A, kw, ts, tile_step=step, apodization="gaussian")[2]
        plan, o = _oracle(A, kw, ts, step)
        out[name] = (A, kw, plan, o, per, F)
    return out


def test_the_cases_walk_what_they_are_there_for(runs):
    for name, ((th, tw), (sy, sx)) in CASES.items():
        A, _, plan, o, _, F = runs[name]
        h, w = A.data_small.shape
        assert plan["tile_grid"] == GRIDS[name] == o["corr"].shape[:2] == F.corr.shape[:2]
        assert sy < th and sx < tw and th % sy and tw % sx  # windows that overlap, by a step that does not divide them
        r, c = F.tile_slices[-1][-1]
        assert (r.stop, c.stop) == (h, w) and r.stop - r.start < th and c.stop - c.start < tw  # ragged on both axes
    assert len(runs["a"][1]["lag_drot"]) == 3  # three rotation planes
    dx = np.asarray(runs["c"][1]["lag_dx"])
    assert (np.abs(np.diff(dx)) > 15).sum() == 4 and len(dx) == 6  # ragged dx groups


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(CASES))
def test_stepped_windows_against_the_oracle(name, method, runs):
    _, _, _, o, per, _ = runs[name]
    corr, counts = per[method]
    key, nkey = KEYS[method]
    assert corr.shape == counts.shape == o[key].shape
    assert np.array_equal(counts, o[nkey])
    _check(corr, o[key], method, f"{name} windows {CASES[name]}")


@pytest.mark.parametrize("name", list(CASES))
def test_apodized_windows_against_the_oracle(name, runs):
    A, _, plan, o, per, F = runs[name]
    assert np.array_equal(F.n_samples, o["count"]) and np.array_equal(F.n_samples, per["correlation"][1])  # n, not W
    assert np.array_equal(F.window[0], plan["window"][0]) and np.array_equal(F.window[1], plan["window"][1])
    _check(F.corr, o["wcorr"], "correlation", f"{name} apodized {CASES[name]}")
    _check_weights(F.weight_sums, o["weight"], name)
    assert np.all(F.weight_sums <= F.n_samples) and not np.array_equal(F.corr, per["correlation"][0], equal_nan=True)
    assert set(A.last_timing) == {"prepare_ms", "pass0_ms", "pass1_ms"}


def _plain(large, small):
    return AlignmentPixels((large, dict(TC.HDR)), 0, (small, dict(TC.HDR)), 0)


def _all_modes(A, kw, ts, step, label, ties):
    first = _local(A, kw, ts, tile_step=step)
    plan, o = _oracle(A, kw, ts, step)
    for m in METHODS:
        corr, n, _ = first if m == "correlation" else _local(A, kw, ts, m, tile_step=step)
        key, nkey = KEYS[m]
        assert np.array_equal(n, o[nkey])
        _check(corr, o[key], m, label, ties=ties)
    F = _local(A, kw, ts, tile_step=step, apodization="gaussian")[2]
    assert np.array_equal(F.n_samples, o["count"])
    _check(F.corr, o["wcorr"], "correlation", label + " apodized", ties=ties)
    _check_weights(F.weight_sums, o["weight"], label)
    return o


def test_a_window_of_two_column_bands():
    """The 3 x (band + 5) image of tests/test_gpu_pxlshift_scores.py::test_second_column_band in windows of (3, band + 2) at
    step (3, 3): two windows, [0, band + 2) and [3, band + 5), each of a second column band of two columns."""
    rng = np.random.default_rng(20)
    small = rng.uniform(1.0, 9.0, (3, BAND + 5))
    large = rng.uniform(1.0, 9.0, (9, BAND + 17))
    for img, n in ((small, 7), (large, 19)):
        img[rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)] = np.nan
    small[1, BAND + 2] = large[4, BAND + 9] = np.nan  # (inside the second band too)
    A = _plain(large, small)
    kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    o = _all_modes(A, kw, (3, BAND + 2), (3, 3), "column bands", ties=True)
    assert o["count"].shape == (1, 2, 5, 3, 1) and o["count"].min() > 3 * BAND - 60


def test_a_window_of_two_row_bands(runs):
    """Case b in windows of (70, 40) at step (70, 30): 40 columns give bands of 51 rows, a second band of 19; four windows,
    the last one [90, 130)."""
    A, kw = runs["b"][:2]
    assert A.data_small.shape == (70, 130) and BAND // 40 == 51
    o = _all_modes(A, kw, (70, 40), (70, 30), "row bands", ties=False)
    assert o["count"].shape[:2] == (1, 4)


# ------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(CASES))
def test_a_step_of_the_tile_shape_is_the_disjoint_call(name, method, runs):
    A, kw = runs[name][:2]
    ts = CASES[name][0]
    corr, n, F0 = _local(A, kw, ts, method)
    corr2, n2, F = _local(A, kw, ts, method, tile_step=ts)
    assert np.array_equal(corr2, corr, equal_nan=True) and np.array_equal(n2, n)  # bit for bit
    assert F.tile_slices == F0.tile_slices and F.weight_sums is None
    # and through the new call itself (the package sends such a plan to coreg_pixels_sweep_tiles)
    plan = A._last_plan
    hnd = _lib.shared_handle(-1)
    cube = hnd.pixels_sweep_windows(plan, plan["method_code"], tile_step=ts)
    assert np.array_equal(cube, corr, equal_nan=True) and np.array_equal(hnd.pixels_last_tile_counts(cube.shape), n)


def test_a_window_on_a_disjoint_tile_has_its_bits(runs):
    """Case a, tile (10, 9), step (5, 9): windows [0, 10), [5, 15), [10, 20), [15, 25) -- windows 0 and 2 are tiles 0 and 1
    of the disjoint call (the ragged tile [20, 25) lies inside the last window: the grid rule gives it none of its own)."""
    A, kw = runs["a"][:2]
    for m in METHODS:
        tiles, nt, _ = _local(A, kw, (10, 9), m)
        wins, nw, F = _local(A, kw, (10, 9), m, tile_step=(5, 9))
        assert wins.shape[:2] == (4, 3) and tiles.shape[:2] == (3, 3)
        assert F.tile_slices[2][1] == (slice(10, 20), slice(9, 18))
        assert np.array_equal(wins[[0, 2]], tiles[[0, 1]], equal_nan=True) and np.array_equal(nw[[0, 2]], nt[[0, 1]])


def test_tables_of_ones(runs):
    for name, (ts, step) in CASES.items():
        A, kw, _, _, per, _ = runs[name]
        corr, n, F = _local(A, kw, ts, tile_step=step, apodization=(np.ones(ts[0]), np.ones(ts[1])))
        assert np.array_equal(n, per["correlation"][1]) and np.array_equal(F.weight_sums, n)  # sums of ones are exact
        _check(corr, per["correlation"][0], "correlation", f"{name} tables of ones")
        same = np.array_equal(corr, per["correlation"][0], equal_nan=True)
        print(name, "tables of ones: the bits of the unapodized call", "agree" if same else "do not agree")


def test_batching_invariance(runs):
    """Case b's cubes, counts and weight sums in one call, and cut into three calls along dx times two along dy."""
    A, kw, _, _, per, F = runs["b"]
    ts, step = CASES["b"]
    dx, dy = np.asarray(kw["lag_dx"]), np.asarray(kw["lag_dy"])
    for apod, whole in ((None, per["correlation"] + (None,)), ("gaussian", (F.corr, F.n_samples, F.weight_sums))):
        cols = [[], [], []]
        for sx in (slice(0, 7), slice(7, 12), slice(12, None)):
            parts = []
            for sy in (slice(0, 9), slice(9, None)):
                G = _local(A, dict(kw, lag_dx=dx[sx], lag_dy=dy[sy]), ts, tile_step=step, apodization=apod)[2]
                parts.append((G.corr, G.n_samples, G.weight_sums))
            for k in range(3):
                if whole[k] is not None:
                    cols[k].append(np.concatenate([p[k] for p in parts], axis=3))
        for k in range(3):
            if whole[k] is not None:
                assert np.array_equal(np.concatenate(cols[k], axis=2), whole[k], equal_nan=True), (apod, k)


# --------------------------------------------------------------------------------------------------- NaN and state
def test_windows_away_from_an_all_nan_window(runs, tmp_path):
    """Window (0, 1) of case a, rows [0, 10) x columns [5, 14), without a finite pixel (unrotated planes): its entries are
    NaN, its counts and weight sums 0, it is not valid; the windows that share no pixel with it -- rows from 12 on, columns
    from 15 on -- keep their bits."""
    A0, kw0 = runs["a"][:2]
    kw = dict(kw0, lag_drot=np.array([0.0]))
    ts, step = CASES["a"]
    A, _ = Cs.make("a", tmp_path)
    A.data_small[0:10, 5:14] = np.nan
    away = np.zeros(GRIDS["a"], dtype=bool)
    away[3:, :] = True
    away[:, 3] = True
    for apod in (None, "gaussian"):
        B = _local(A0, kw, ts, tile_step=step, apodization=apod)[2]
        F = A.find_local_shifts(**kw, tile_shape=ts, tile_step=step, apodization=apod, sub_lag=False)
        assert np.isnan(F.corr[0, 1]).all() and not F.n_samples[0, 1].any() and not F.valid[0, 1]
        assert np.isnan(F.shift_dx[0, 1]) and (F.best_index[0, 1] == -1).all()
        assert np.isfinite(B.corr[0, 1]).all() and F.valid[away].all()
        assert np.array_equal(F.corr[away], B.corr[away], equal_nan=True) and np.array_equal(F.n_samples[away], B.n_samples[away])
        if apod:
            assert not F.weight_sums[0, 1].any() and np.array_equal(F.weight_sums[away], B.weight_sums[away])


def _code(fn, *args, **kw):
    with pytest.raises(_lib.CoregError) as e:
        fn(*args, **kw)
    return e.value.code


def test_state_and_refusals(runs):
    A, kw = runs["c"][:2]
    ts, step = CASES["c"]
    plan = A.host_plan(**kw, tile_shape=ts, tile_step=step, apodization="gaussian")
    bare = dict(plan, window=None)
    shape5 = plan["tile_grid"] + (len(plan["lag_dx"]), len(plan["lag_dy"]), len(plan["lag_drot"]))
    code = plan["method_code"]
    with _lib.CoregHandle(0) as hnd:
        assert _code(hnd.pixels_last_tile_weights, shape5) == _lib.COREG_ESTATE  # a fresh handle
        hnd.pixels_set_large(A.data_large)
        hnd.pixels_set_small(A.data_small)
        cube = hnd.pixels_sweep(plan, code)
        counts = hnd.pixels_last_counts(cube.shape)
        assert _code(hnd.pixels_last_tile_weights, shape5) == _lib.COREG_ESTATE  # after an untiled sweep
        stepped = hnd.pixels_sweep_tiles(bare, code)
        assert stepped.shape == shape5
        n = hnd.pixels_last_tile_counts(shape5)
        assert _code(hnd.pixels_last_tile_weights, shape5) == _lib.COREG_ESTATE  # after a tiled sweep without tables
        assert _code(hnd.pixels_last_counts, cube.shape) == _lib.COREG_ESTATE
        apod = hnd.pixels_sweep_tiles(plan, code)
        W = hnd.pixels_last_tile_weights(shape5)
        assert np.array_equal(hnd.pixels_last_tile_counts(shape5), n) and np.all(W <= n) and W.max() > 0
        assert _code(hnd.pixels_last_counts, cube.shape) == _lib.COREG_ESTATE  # after an apodized sweep
        assert set(hnd.pixels_last_timing()) == {"prepare_ms", "pass0_ms", "pass1_ms"}
        assert not np.array_equal(apod, stepped, equal_nan=True)
        # an untiled sweep after an apodized one has its usual bits
        assert np.array_equal(hnd.pixels_sweep(plan, code), cube, equal_nan=True)
        assert np.array_equal(hnd.pixels_last_counts(cube.shape), counts)
        assert _code(hnd.pixels_last_tile_weights, shape5) == _lib.COREG_ESTATE
        hnd.pixels_sweep_tiles(plan, code)
        hnd.pixels_set_small(A.data_small)
        assert _code(hnd.pixels_last_tile_weights, shape5) == _lib.COREG_ESTATE  # after a new image
        assert _code(hnd.pixels_last_tile_counts, shape5) == _lib.COREG_ESTATE
        # refusals by error code: the step
        for bad in ((0, 5), (4, 0), (11, 5), (4, 10), (-1, 5)):
            assert _code(hnd.pixels_sweep_windows, plan, code, tile_step=bad) == _lib.COREG_EINVAL
        # ... the tables
        wy, wx = plan["window"]
        for k, v in ((3, -0.5), (0, np.nan), (9, np.inf)):
            t = wy.copy()
            t[k] = v
            assert _code(hnd.pixels_sweep_windows, plan, code, tile_step=step, window=(t, wx)) == _lib.COREG_EINVAL
            t = wx.copy()
            t[min(k, 8)] = v
            assert _code(hnd.pixels_sweep_windows, plan, code, tile_step=step, window=(wy, t)) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_windows, plan, code, tile_step=step, window=(np.zeros(10), wx)) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_windows, plan, code, tile_step=step, window=(wy, np.zeros(9))) == _lib.COREG_EINVAL
        # ... tables with another method, an unknown method, the unmasked residus
        mplan = A.host_plan(**kw, tile_shape=ts, tile_step=step, method=MI)
        assert _code(hnd.pixels_sweep_windows, mplan, _lib.METHOD_MUTUAL_INFORMATION, tile_step=step, window=(wy, wx)) == \
            _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_windows, plan, _lib.METHOD_RESIDUS_MASKED, tile_step=step, window=(wy, wx)) == \
            _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_windows, plan, 7, tile_step=step) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_sweep_windows, plan, _lib.METHOD_RESIDUS, tile_step=step) == _lib.COREG_ENOTIMPL
        # ... one table without the other (the C call itself)
        p = _lib.PixelsPlan()
        out = np.empty(shape5)
        assert hnd._lib.coreg_pixels_sweep_windows(hnd._h, p, code, 10, 9, 4, 5, wy.ctypes.data, None,
                                                   out.ctypes.data) == _lib.COREG_EINVAL
        # 300 x 300 pixels in windows of (2, 2) at step (1, 1): 299 x 299 windows, more than 65535 planes x windows
        big = _plain(np.ones((310, 310)), np.ones((300, 300)))
        bplan = big.host_plan([0], [0], [0.0], tile_shape=(2, 2), tile_step=(1, 1))
        assert bplan["tile_grid"] == (299, 299)
        hnd.pixels_set_large(big.data_large)
        hnd.pixels_set_small(big.data_small)
        assert _code(hnd.pixels_sweep_tiles, bplan, bplan["method_code"]) == _lib.COREG_EINVAL
        assert _code(hnd.pixels_last_tile_counts, (1,)) == _lib.COREG_ESTATE


# ------------------------------------------------------------------------------------------------------ end to end
def test_two_drift_scene_end_to_end():
    A, kw, ts, want = TC.two_drift_object()
    lag = kw["lag_dx"]
    for apod in (None, (5.0, 6.0)):
        F = A.find_local_shifts(**kw, tile_shape=ts, tile_step=(10, 12), apodization=apod, sub_lag=False)
        assert F.corr.shape == (3, 3, 9, 9, 1) and F.valid.all() and (F.weight_sums is None) == (apod is None)
        for ty in range(3):
            for tx, half in ((0, want[0][0]), (2, want[0][1])):  # column starts 0 and 24: one half each
                top = np.sort(F.corr[ty, tx].ravel())[-2:]
                print(apod, (ty, tx), "best", F.shift_dx[ty, tx], F.shift_dy[ty, tx], "top two", top[1], top[0])
                assert (lag[F.best_index[ty, tx, 0]], lag[F.best_index[ty, tx, 1]]) == half
                assert (F.shift_dx[ty, tx], F.shift_dy[ty, tx]) == half and top[1] - top[0] >= 0.1
        assert F.tile_centres[0, :, 0].tolist() == [11.5, 23.5, 35.5] and F.tile_centres[:, 0, 1].tolist() == [9.5, 19.5, 29.5]
        got, disp = F.destretch(A.data_small, return_displacement=True)
        assert np.array_equal(got, D.field_destretch(F, A.data_small), equal_nan=True)  # the rule of the disjoint field
        u, v = F.node_shifts()
        assert disp.shape == (2, 40, 48) and disp[0].min() >= u.min() - 1e-12 and disp[0].max() <= u.max() + 1e-12
        assert disp[0][:, :12].max() > disp[0][:, 36:].min() + 2.5  # the halves lie 3 pixels apart in dx
        with pytest.raises(ValueError, match="nearest"):
            F.destretch(A.data_small, interpolation="nearest")
    with pytest.raises(ValueError, match="apodization"):
        A.find_local_shifts(**kw, tile_shape=ts, apodization="gaussian", method="residus_masked")
