"""GPU tests of method 'residus_masked', of the per-lag sample counts (coreg_last_counts / coreg_multi_last_counts) and of
`min_overlap`, on every sweep path, against the numpy oracle of tests/masked_scores_oracle.py.

Tolerances are the ones the project applies to 'residus' (tests/test_gpu_parity.py::test_method_residus,
tests/test_gpu_context_fuzz.py): |got - want| <= 1e-10 max|want| on the Carrington path, 1e-5 relative on the
helioprojective and plate-carree paths (float32 arithmetic of the reference), 1e-8 relative for the context sweep.  The
counts are integers and must be equal exactly."""
import warnings

import numpy as np
import pytest

from tests import helpers as H
from tests import masked_scores_oracle as M

pytestmark = pytest.mark.gpu

CARR_RTOL, HELIO_RTOL, CTX_RTOL = 1e-10, 1e-5, 1e-8


def _lags(n1=5, n2=5, step=2.0, c1=17.0, c2=-9.0, cdelt1=None, cdelt2=None, crota=None):
    return (c1 + step * (np.arange(n1) - n1 // 2), c2 + step * (np.arange(n2) - n2 // 2), cdelt1, cdelt2, crota)


def assert_masked(got, want, rtol, what, per_entry=False):
    """Same NaN pattern; |got - want| <= rtol max|want| (or rtol |want| entry by entry); same argmin."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs\n{got}\n{want}"
    fin = np.isfinite(want)
    if not fin.any():
        return
    err = np.abs(got[fin] - want[fin])
    bound = rtol * (np.abs(want[fin]) if per_entry else np.abs(want[fin]).max())
    print(f"\n[masked scores] {what}: max error / bound = {np.max(err / bound):.3e}")
    assert (err <= bound).all(), f"{what}: {np.max(err / bound):.3e} x the bound"
    best = np.argsort(want[fin])
    if best.size > 1 and want[fin][best[1]] - want[fin][best[0]] > 2 * rtol * np.abs(want[fin]).max():
        assert np.nanargmin(got) == np.nanargmin(want), f"{what}: argmin differs"


def assert_counts(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert np.array_equal(got, want, equal_nan=True), f"{what}: counts differ\n{got}\n{want}"


def carr_state(small, hs, large, hl, lags, shape, lon=H.CARR_LON, lat=H.CARR_LAT):
    return H.oracle_state(small, hs, large, hl, lags, shape=list(shape), lonlims=list(lon), latlims=list(lat),
                          solar_r=(1.004,))


@pytest.fixture(scope="module")
def usual():
    """The usual Carrington grid (two tiles), 5 x 5 lags, with the oracle's sweep computed once."""
    small, hs, large, hl, _ = H.scene()
    lags = _lags(5, 5)
    want = M.sweep(carr_state(small, hs, large, hl, lags, (48, 40)), "carrington")
    return small, hs, large, hl, lags, want


def carr_sweep(h, small, hs, large, hl, lags, shape, method, lon=H.CARR_LON, lat=H.CARR_LAT, prepare=True, **kw):
    from euispice_coreg_amd import _lib
    grid = _lib.Grid(lon, lat, shape)
    if prepare:
        h.set_small(small)
        h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
    return h.sweep_carrington(hs, grid, 1.004, _lib.LagSet(*lags), method=method, **kw)


# ---- 1. Carrington, the usual grid ------------------------------------------------------------------------------------
def test_carrington_usual_grid(gpu_handle, usual):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, lags, want = usual
    assert np.isfinite(want["masked"]).all() and want["poisoned"].sum() == 0
    assert want["count"].min() == 780 and want["count"].max() == 788  # of 1920 grid points
    got = carr_sweep(gpu_handle, small, hs, large, hl, lags, (48, 40), _lib.METHOD_RESIDUS_MASKED)
    assert_counts(gpu_handle.last_counts(), want["finite_terms"], "carrington, masked")
    assert_masked(got, want["masked"], CARR_RTOL, "carrington, usual grid")
    # the reference's residus is still NaN there, with the same number of finite terms behind it
    got = carr_sweep(gpu_handle, small, hs, large, hl, lags, (48, 40), _lib.METHOD_RESIDUS, prepare=False)
    assert np.isnan(got).all()
    assert_counts(gpu_handle.last_counts(), want["finite_terms"], "carrington, residus")
    # and the Pearson sweep reports the samples of its six sums: the co-finite points
    got = carr_sweep(gpu_handle, small, hs, large, hl, lags, (48, 40), _lib.METHOD_CORRELATION, prepare=False)
    assert np.isfinite(got).all()
    assert_counts(gpu_handle.last_counts(), want["count"], "carrington, correlation")
    # a slice of the lag range: the counts have the layout of the slice
    part = carr_sweep(gpu_handle, small, hs, large, hl, lags, (48, 40), _lib.METHOD_RESIDUS_MASKED, prepare=False,
                      lag_begin=3, lag_end=19)
    assert_masked(part, want["masked"].ravel()[3:19], CARR_RTOL, "carrington, lag slice")
    assert_counts(gpu_handle.last_counts(), want["finite_terms"].ravel()[3:19], "carrington, lag slice")


# ---- 2. Carrington, full overlap ----------------------------------------------------------------------------------------
def test_carrington_full_overlap_equals_residus_bit_for_bit(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene(nan_frac=0.0)
    lags = _lags(3, 3)
    lon, lat, shape = (243.0, 249.0), (2.0, 8.0), (40, 36)
    masked = carr_sweep(gpu_handle, small, hs, large, hl, lags, shape, _lib.METHOD_RESIDUS_MASKED, lon, lat)
    n_masked = gpu_handle.last_counts()
    plain = carr_sweep(gpu_handle, small, hs, large, hl, lags, shape, _lib.METHOD_RESIDUS, lon, lat, prepare=False)
    assert np.isfinite(plain).all() and np.array_equal(masked, plain)
    assert (n_masked == 1440).all() and (gpu_handle.last_counts() == 1440).all()
    want = M.sweep(carr_state(small, hs, large, hl, lags, shape, lon, lat), "carrington")
    assert_masked(masked, want["masked"], CARR_RTOL, "carrington, full overlap")


# ---- 3. wide lags: the counts, and min_overlap through the class ------------------------------------------------------
def test_wide_lags_counts_and_min_overlap(gpu_handle, tmp_path):
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.hdrshift import Alignment, AlignmentResults
    from euispice_coreg_amd.utils import fits_io
    small, hs, large, hl, _ = H.scene()
    wide = 17.0 + np.arange(-600.0, 601.0, 150.0)
    lags = (wide, [-9.0], None, None, None)
    want = M.sweep(carr_state(small, hs, large, hl, lags, (48, 40)), "carrington")
    assert want["count"].ravel().astype(int).tolist() == [448, 560, 671, 786, 782, 778, 779, 702, 580]
    got = carr_sweep(gpu_handle, small, hs, large, hl, lags, (48, 40), _lib.METHOD_RESIDUS_MASKED)
    assert_counts(gpu_handle.last_counts(), want["finite_terms"], "wide lags")
    assert_masked(got, want["masked"], CARR_RTOL, "wide lags")
    # on files, through the class (the scene's pixels are float32-exact: the files hold what the oracle saw)
    for img in (small, large):
        assert np.array_equal(img.astype(np.float32), img, equal_nan=True)
    assert want["poisoned"].sum() == 0
    ps, pl = str(tmp_path / "small.fits"), str(tmp_path / "large.fits")
    fits_io.write_images(ps, [(None, {}), (small.astype(np.float32), hs)])
    fits_io.write_images(pl, [(None, {}), (large.astype(np.float32), hl)])
    kw = dict(lonlims=H.CARR_LON, latlims=H.CARR_LAT, shape=(48, 40))
    keep = want["count"] >= 0.9 * 786
    assert keep.sum() == 4
    for method, best in (("residus_masked", "min"), ("correlation", "max")):
        A = Alignment(pl, ps, lag_crval1=wide, lag_crval2=[-9.0], lag_cdelt1=None, lag_cdelt2=None, lag_crota=None,
                      min_overlap=0.9)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (one CRVAL2 lag: no Gaussian fit)
            res = A.align_using_carrington(method=method, **kw)
        assert isinstance(res, AlignmentResults) and res.best == best
        assert res.corr.shape == (9, 1, 1, 1, 1, 1) == np.shape(res.n_samples) == np.shape(A.last_counts)
        assert_counts(res.n_samples, want["count"], f"Alignment {method}")
        assert np.array_equal(np.isfinite(res.corr), keep), (method, res.corr.ravel())
        if method == "residus_masked":
            assert_masked(res.corr[keep], want["masked"][keep], CARR_RTOL, "Alignment residus_masked")
            assert tuple(int(v) for v in res.max_index) == np.unravel_index(
                np.nanargmin(np.where(keep, want["masked"], np.nan)), keep.shape)
        # return_type='corr': the floor is applied there too
        A = Alignment(pl, ps, lag_crval1=wide, lag_crval2=[-9.0], lag_cdelt1=None, lag_cdelt2=None, lag_crota=None,
                      min_overlap=700)
        corr = A.align_using_carrington(method=method, return_type="corr", **kw)
        assert np.array_equal(np.isfinite(corr), want["count"] >= 700) and np.isfinite(corr).sum() == 5
    # the default changes nothing; a floor nothing meets says so
    A = Alignment(pl, ps, lag_crval1=wide, lag_crval2=[-9.0], lag_cdelt1=None, lag_cdelt2=None, lag_crota=None)
    corr = A.align_using_carrington(method="residus_masked", return_type="corr", **kw)
    assert np.isfinite(corr).all() and np.array_equal(corr.ravel(), got)
    A = Alignment(pl, ps, lag_crval1=wide, lag_crval2=[-9.0], lag_cdelt1=None, lag_cdelt2=None, lag_crota=None,
                  min_overlap=1000)
    with pytest.raises(ValueError, match="leaves no lag-point"):
        A.align_using_carrington(method="residus_masked", **kw)


# ---- 4. helioprojective, parallel semantics ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helio_scene():
    return H.scene(small_n=64, large_n=96)


ZERO_LAGS = ([-4.0, -2.0, 0.0, 2.0], [-2.0, 0.0, 2.0], None, None, None)  # through exactly 0.0 on both axes


def helio_sweep(h, small, hs, large, hl, lags, order, method, prepare=True):
    from euispice_coreg_amd import _lib
    if prepare:
        h.set_small(small)
        h.prepare_reference_helioprojective(large, hl, hs, order)
    return h.sweep_helioprojective(hs, hs, _lib.LagSet(*lags), order=order, method=method)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_helioprojective_parallel_semantics_through_zero(gpu_handle, helio_scene, order):
    """The zero lag takes the border pass, the odd orders the parity and tap passes: their residus branches carry the
    masked method's terms like the sweep's."""
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = helio_scene
    want = M.sweep(H.oracle_state(small, hs, large, hl, ZERO_LAGS, order=order), "helioprojective")
    assert np.isfinite(want["masked"]).all() and want["poisoned"].sum() == 0
    if order == 2:
        assert set(want["count"].ravel().astype(int).tolist()) >= {3822}  # of 4096
    got = helio_sweep(gpu_handle, small, hs, large, hl, ZERO_LAGS, order, _lib.METHOD_RESIDUS_MASKED)
    assert_counts(gpu_handle.last_counts(), want["finite_terms"], f"helioprojective order {order}")
    assert_masked(got, want["masked"], HELIO_RTOL, f"helioprojective order {order}", per_entry=True)
    got = helio_sweep(gpu_handle, small, hs, large, hl, ZERO_LAGS, order, _lib.METHOD_CORRELATION, prepare=False)
    assert_counts(gpu_handle.last_counts(), want["count"], f"helioprojective order {order}, correlation")
    assert np.isnan(helio_sweep(gpu_handle, small, hs, large, hl, ZERO_LAGS, order, _lib.METHOD_RESIDUS,
                                prepare=False)).all()


# ---- 5. serial semantics, a poisoned term -----------------------------------------------------------------------------
def test_serial_semantics_poisoned_term(gpu_handle, helio_scene):
    """One exact 0 in the reference image on its own grid (set_reference_on_grid), under a finite sample at some lags and
    outside the overlap at others: NaN wherever the mask holds it -- (A - B) / sqrt(0) is infinite and numpy's std of that
    is NaN -- a number elsewhere; the counts hold the finite terms only."""
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = helio_scene
    lags = ([-60.0, 0.0, 60.0], [0.0, 40.0], None, None, None)
    ls = _lib.LagSet(*lags)
    clean = M.sweep(H.oracle_state(small, hs, large, hl, lags), "helioprojective", parallelism=False)
    assert np.isfinite(clean["masked"]).all()
    z = np.array(large, dtype=np.float64)
    z[50, 42] = 0.0
    want = M.sweep(H.oracle_state(small, hs, z, hl, lags), "helioprojective", parallelism=False)
    hit = want["poisoned"] > 0
    assert hit.any() and not hit.all() and want["poisoned"].max() == 1
    assert np.array_equal(np.isnan(want["masked"]), hit) and np.array_equal(want["count"], clean["count"])
    assert np.array_equal(want["finite_terms"], clean["count"] - hit)
    gpu_handle.set_small(small)
    gpu_handle.set_reference_on_grid(z)
    got = gpu_handle.sweep_helioprojective(hl, hs, ls, method=_lib.METHOD_RESIDUS_MASKED).reshape(hit.shape)
    assert np.array_equal(np.isnan(got).ravel(), hit.ravel()), got
    assert_counts(gpu_handle.last_counts(), want["finite_terms"], "serial semantics, poisoned")
    assert_masked(got, want["masked"], HELIO_RTOL, "serial semantics, poisoned", per_entry=True)
    # without the zero: a number everywhere
    gpu_handle.set_reference_on_grid(np.array(large, dtype=np.float64))
    got = gpu_handle.sweep_helioprojective(hl, hs, ls, method=_lib.METHOD_RESIDUS_MASKED)
    assert_counts(gpu_handle.last_counts(), clean["count"], "serial semantics")
    assert_masked(got, clean["masked"], HELIO_RTOL, "serial semantics", per_entry=True)


# ---- 6. plate carree ----------------------------------------------------------------------------------------------------
def test_plate_carree_through_the_class(tmp_path):
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.hdrshift import Alignment
    from euispice_coreg_amd.utils import fits_io
    from oracle import coreg_oracle as O
    small, hs, large, hl, truth = synthetic.make_car_scene()
    ps, pl = str(tmp_path / "small_car.fits"), str(tmp_path / "large_car.fits")
    fits_io.write_images(ps, [(None, {}), (small, hs)])
    fits_io.write_images(pl, [(None, {}), (large, hl)])
    lag1, lag2 = np.arange(15.0, 135.0, 40.0), np.arange(-85.0, 35.0, 40.0)  # arcsec; the maps are in degrees
    A = Alignment(pl, ps, lag_crval1=lag1, lag_crval2=lag2, lag_cdelt1=None, lag_cdelt2=None, lag_crota=None,
                  parallelism=True, small_fov_value_max=2900.0, reprojection_order=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = A.align_using_initial_carrington(method="residus_masked")
    sm = small.astype(np.float64)
    O.set_threshold_minmax_to_nan(sm, None, 2900.0)
    st = H.oracle_state(sm, hs, large.astype(np.float64), hl, (lag1 / 3600.0, lag2 / 3600.0, None, None, None),
                        unit_lag="deg")
    want = M.sweep(st, "initial_carrington", use_ang2pipi=False)
    assert np.isfinite(want["masked"]).all() and want["poisoned"].sum() == 0
    assert res.best == "min" and res.corr.shape == (3, 3, 1, 1, 1, 1) == np.shape(res.n_samples)
    assert_counts(res.n_samples, want["finite_terms"], "plate carree")
    assert_masked(res.corr, want["masked"], HELIO_RTOL, "plate carree", per_entry=True)
    assert tuple(int(v) for v in res.max_index) == np.unravel_index(np.argmin(want["masked"]), want["masked"].shape)


# ---- 7. grid shares -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 3])
def test_grid_shares_add_up_to_the_oracle(gpu_handle, usual, helio_scene, W):
    """Every rank sweeps all lags over its share of the grid; the six sums -- the poisoned count among them -- are added
    and finalised (emulated on one GPU, as tests/test_gpu_parity.py does)."""
    from euispice_coreg_amd import _lib

    def shared(run, n_out):
        total = None
        try:
            for r in range(W):
                gpu_handle.set_point_shard(r, W)
                assert np.isnan(run()).all()
                s = gpu_handle.copy_sums()
                total = s if total is None else total + s
            return gpu_handle.finalize_sums(total, n_out), gpu_handle.last_counts()
        finally:
            gpu_handle.set_point_shard(0, 1)

    small, hs, large, hl, lags, want = usual
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    ls = _lib.LagSet(*lags)
    gpu_handle.set_small(small)
    gpu_handle.prepare_reference_carrington(large, hl, grid, 1.004, 2)
    got, n = shared(lambda: gpu_handle.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_RESIDUS_MASKED), ls.size)
    assert_counts(n, want["finite_terms"], f"carrington, {W} shares")
    assert_masked(got, want["masked"], CARR_RTOL, f"carrington, {W} shares")
    small, hs, large, hl, _ = helio_scene
    want = M.sweep(H.oracle_state(small, hs, large, hl, ZERO_LAGS, order=3), "helioprojective")
    ls = _lib.LagSet(*ZERO_LAGS)
    gpu_handle.set_small(small)
    gpu_handle.prepare_reference_helioprojective(large, hl, hs, 3)
    got, n = shared(lambda: gpu_handle.sweep_helioprojective(hs, hs, ls, order=3, method=_lib.METHOD_RESIDUS_MASKED),
                    ls.size)
    assert_counts(n, want["finite_terms"], f"helioprojective, {W} shares")
    assert_masked(got, want["masked"], HELIO_RTOL, f"helioprojective, {W} shares", per_entry=True)


# ---- 8. the in-library multi-GPU driver --------------------------------------------------------------------------------
def test_two_logical_devices_through_the_class(monkeypatch, usual):
    """COREG_VIRTUAL_DEVICES=2, Alignment(parallelism=True): grid shares for the 25 lag-points of the usual sweep (device 0
    finalises the added sums), blocks of the lag plane for 24 x 12 (each device's counts scattered into the map)."""
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.hdrshift import Alignment
    small, hs, large, hl, lags, want = usual
    l1, l2 = 17.0 + 1.0 * (np.arange(24) - 12), -9.0 + 1.0 * (np.arange(12) - 6)
    big = M.sweep(carr_state(small, hs, large, hl, (l1, l2, None, None, None), (48, 40)), "carrington")
    monkeypatch.setenv("COREG_VIRTUAL_DEVICES", "2")
    _lib._close_shared()
    try:
        for (a1, a2), w, mode in (((lags[0], lags[1]), want, "points"), ((l1, l2), big, "blocks")):
            for method, key in (("residus_masked", "finite_terms"), ("correlation", "count")):
                A = Alignment((large, hl), (small, hs), lag_crval1=a1, lag_crval2=a2, lag_cdelt1=None, lag_cdelt2=None,
                              lag_crota=None, parallelism=True)
                res = A.align_using_carrington(lonlims=H.CARR_LON, latlims=H.CARR_LAT, shape=(48, 40), method=method)
                assert A.last_stats["n_devices"] == 2 and A.last_sharding == mode
                assert np.shape(res.n_samples) == res.corr.shape == w["masked"].shape
                assert_counts(res.n_samples, w[key], f"two devices, {mode}, {method}")
                if method == "residus_masked":
                    assert_masked(res.corr, w["masked"], CARR_RTOL, f"two devices, {mode}")
                    assert res.best == "min"
    finally:
        _lib._close_shared()


# ---- 9. the iterative-context sweep -------------------------------------------------------------------------------------
def context_case(what):
    """A 5 x 24 raster (three column groups of the kernel, the last one ragged; tests/test_gpu_context_fuzz.py's small
    shape), two frames alternating by column, six lag-points of which the CRVAL2 = 40 arcsec ones move the raster by more
    than its height.  "thresholds": both; "nan pixels": 1 % in the frames and in the SPICE image; "zero context sample": a
    3 x 3 block of exact zeros in a frame under the raster's middle point at zero lag."""
    from oracle import context_oracle as CO
    from oracle import coreg_oracle as O
    from tests import context_cases as CC
    lags = [np.array([-4.0, 0.0, 4.0]) * CC.AS, np.array([0.0, 40.0]) * CC.AS, None, None, None]
    case = CC.make_case(7000, gW=5, gH=24, method="residus", order=2, semantics=CO.INTENDED, n_frames=2,
                        col_mode="every", thresholds="both" if what == "thresholds" else "none",
                        nan_frac=0.01 if what == "nan pixels" else 0.0, zeros=False, frame_dtype=np.float64,
                        spice_dtype=np.float64, lags=lags)
    if what == "zero context sample":
        i, j = 2, 12
        f = int(case["col_frame"][i])
        ctx, _, _ = CO.lag_headers(case["target4"], case["hdr_small"], 0.0, 0.0, 0.0, 0.0, 0.0)
        ox, oy, _, _ = O.wcslib_pixel_to_pixel(ctx, case["frame_headers"][f], [float(i)], [float(j)])
        cx, cy = int(np.rint(ox[0])), int(np.rint(oy[0]))
        case["frames"][f][cy - 1:cy + 2, cx - 1:cx + 2] = 0.0
    return case


def context_gpu(h, case, method):
    from euispice_coreg_amd import _lib
    from tests import context_cases as CC
    CC.upload(h, case)
    ls = _lib.LagSet(*case["lags"])
    out = h.sweep_context(case["target4"], case["hdr_small"], case["col_frame"], ls, order=case["order"], method=method,
                          vmin=case["vmin"], vmax=case["vmax"])
    return out.reshape(ls.shape), h.last_counts().reshape(ls.shape)


@pytest.mark.parametrize("what", ["thresholds", "nan pixels", "zero context sample"])
def test_context_sweep(what):
    from euispice_coreg_amd import _lib
    case = context_case(what)
    want = M.context_sweep(case)
    hit = want["poisoned"] > 0
    assert np.array_equal(np.isnan(want["masked"]), hit | (want["count"] == 0))
    assert np.isfinite(want["masked"]).any() and hit.any() == (what == "zero context sample")
    h = _lib.CoregHandle(0)
    try:
        got, n = context_gpu(h, case, _lib.METHOD_RESIDUS_MASKED)
        assert_counts(n, want["finite_terms"], f"context, {what}")
        assert_masked(got, want["masked"], CTX_RTOL, f"context, {what}", per_entry=True)
        _, n = context_gpu(h, case, _lib.METHOD_CORRELATION)
        assert_counts(n, want["count"], f"context, {what}, correlation")
    finally:
        h.close()


# ---- 10. the jitter series ----------------------------------------------------------------------------------------------
def test_jitter_series_with_the_masked_residus(tmp_path):
    """Three frames of the jittering series of tests/test_gpu_jitter.py, `residus_masked` with a floor on the overlap:
    every corrected CRVAL within 1.0 arcsec of the injected jitter (that test's bound); the default call still follows
    the oracle's chain."""
    import os
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.jitter_correction import jitter_correction_imagers
    from euispice_coreg_amd.utils import fits_io
    from oracle import coreg_oracle as O
    LON, LAT, SHAPE = (236.0, 256.0), (-4.0, 16.0), (200, 200)
    frames, jit = synthetic.make_series(n_frames=3, n=256, seed=7, jitter_sigma=4.0)
    paths = []
    for k, (img, hdr) in enumerate(frames):
        p = str(tmp_path / f"solo_L2_eui-hrieuv174-image_{k:03d}.fits")
        fits_io.write_images(p, [(None, {}), (img, hdr)])
        paths.append(p)
    lag = np.arange(-12.0, 12.5, 1.0)
    kw = dict(lonlims=LON, latlims=LAT, shape=SHAPE, lag_crval1=lag, lag_crval2=lag, sublist_length=3, overlap=1,
              small_fov_value_max=2800.0)
    out = str(tmp_path / "masked")
    done = jitter_correction_imagers(paths, out, method="residus_masked", min_overlap=0.5, **kw)
    assert [(a, r) for a, r, _ in done] == [(1, 0), (2, 0)]
    for idx, _, res in done:
        assert res.best == "min" and np.shape(res.n_samples) == res.corr.shape == (25, 25, 1, 1, 1, 1)
        assert np.isfinite(res.corr).all() and np.nanmin(res.n_samples) > 30000  # of 40 000 grid points
        hdr_out = fits_io.read_header(os.path.join(out, os.path.basename(paths[idx])), -1)
        d1 = hdr_out["CRVAL1"] - (frames[idx][1]["CRVAL1"] + jit[idx, 0])
        d2 = hdr_out["CRVAL2"] - (frames[idx][1]["CRVAL2"] + jit[idx, 1])
        print(f"\n[masked scores] jitter frame {idx}: corrected CRVAL - injected = ({d1:+.4f}, {d2:+.4f}) arcsec, "
              f"residus at the minimum {np.nanmin(res.corr):.3f}")
        assert abs(d1) < 1.0 and abs(d2) < 1.0
    # the default call: still the Pearson chain of the oracle (tests/test_gpu_jitter.py checks whole maps; here the
    # 5 x 5 patch of the fit about the maximum and forty more lag-points, the oracle's values put in their places)
    from euispice_coreg_amd.hdrshift import AlignmentResults
    out = str(tmp_path / "default")
    done = jitter_correction_imagers(paths, out, **kw)
    assert [(a, r) for a, r, _ in done] == [(1, 0), (2, 0)]
    rng = np.random.default_rng(3)
    for idx, ref, res in done:
        assert res.best == "max"
        img = frames[idx][0].astype(np.float64)
        O.set_threshold_minmax_to_nan(img, None, 2800.0)
        mi = res.max_index
        patch = [(a, b) for a in range(mi[0] - 2, mi[0] + 3) for b in range(mi[1] - 2, mi[1] + 3)
                 if 0 <= a < 25 and 0 <= b < 25]
        subset = np.unique(np.concatenate([[a * 25 + b for a, b in patch], rng.choice(625, 40, replace=False)]))
        st = H.oracle_state(img, frames[idx][1], frames[ref][0].astype(np.float64), frames[ref][1],
                            (lag, lag, [0], [0], [0]), shape=list(SHAPE), lonlims=list(LON), latlims=list(LAT),
                            solar_r=(1.004,))
        want = O.find_best_header_parameters(st, "carrington", lag_subset=subset)
        sel = np.isfinite(want)
        assert sel.sum() == subset.size and np.abs(res.corr[sel] - want[sel]).max() <= 1e-10
        assert want[sel].max() == want[tuple(mi)]
        r = AlignmentResults(np.where(sel, want, res.corr), lag, lag, [0], [0], [0], "arcsec")
        hdr_out = fits_io.read_header(os.path.join(out, os.path.basename(paths[idx])), -1)
        assert abs(hdr_out["CRVAL1"] - (frames[idx][1]["CRVAL1"] + r.shift_arcsec[0])) < 1e-3
        assert abs(hdr_out["CRVAL2"] - (frames[idx][1]["CRVAL2"] + r.shift_arcsec[1])) < 1e-3
