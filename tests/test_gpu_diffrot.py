"""GPU tests of the differential rotation on the Carrington path (`differential_rotation="intended"`,
coreg_set_reference_rotation / coreg_set_small_rotation):

  * `resample_carrington` with a rotation against the REFERENCE's own `CarringtonTransform(reference_date=...,
    rate_wave=band)` + `Rectifier` (tests/golden/rectify_diffrot_golden.npz), under the rule of tests/test_gpu_parity.py;
  * `Alignment(differential_rotation="intended")` and a `jitter_correction_imagers` session against the reference's
    `align_using_carrington` with its band table given the integer keys it lacks
    (tests/golden/diffrot_alignment_golden.{npz,json}), the default call against the unpatched reference;
  * the whole-tile skip of k_precompute, a rotation set and cleared, and the multi-device driver, each against the
    plain path, map for map."""
import json
import os
import warnings

import numpy as np
import pytest

from tests import helpers as H
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

ROT_304_2D = (2.0, 14.51, -3.12, 0.34)


@pytest.fixture(scope="module")
def rectify_diffrot():
    return np.load(os.path.join(GOLDEN, "rectify_diffrot_golden.npz"))


@pytest.fixture(scope="module")
def alignment_golden(tmp_path_factory):
    from euispice_coreg_amd.utils import fits_io
    g = np.load(os.path.join(GOLDEN, "diffrot_alignment_golden.npz"))
    with open(os.path.join(GOLDEN, "diffrot_alignment_golden.json")) as f:
        m = json.load(f)
    d = tmp_path_factory.mktemp("diffrot_alignment")
    paths = {}
    for name, c in m["cases"].items():
        ps, pl = str(d / f"{name}_small.fits"), str(d / f"{name}_large.fits")
        fits_io.write_images(ps, [(None, {}), (g["small"], c["hdr_small"])])
        fits_io.write_images(pl, [(None, {}), (g["large"], c["hdr_large"])])
        paths[name] = (ps, pl)
    return g, m, paths


RECTIFY_CASES = ["b171_p015d", "b195_m2d", "b304_p10min_o1", "b284_m2d_limb", "b304_p015d_highlat", "b171_m2d_highlat_o1",
                 "b171_m2d_crota2", "none_m2d"]


def test_every_rectify_case_is_run(rectify_diffrot):
    assert sorted({k.split("/")[0] for k in rectify_diffrot.files}) == sorted(RECTIFY_CASES)


@pytest.mark.parametrize("case", RECTIFY_CASES)
def test_rotated_resample_matches_reference_golden(gpu_handle, rectify_diffrot, case):
    from euispice_coreg_amd import _lib
    from tests.conftest import rectify_case
    g = rectify_diffrot
    c = rectify_case(g, case)
    rot = (float(g[case + "/delta_t"]),) + tuple(float(v) for v in g[case + "/coeffs"])
    gpu_handle.set_small(c["image"])
    grid = _lib.Grid(c["lonlims"], c["latlims"], c["shape"], numpy_lat_trig=True)
    gpu_handle.set_rotation("small", rot)
    try:
        out = gpu_handle.resample_carrington(c["hdr"], grid, c["solar_r"], order=c["order"])
    finally:
        gpu_handle.set_rotation("small", None)
    want = c["resampled"]
    assert out.shape == want.shape
    # points whose coordinate sits within 1e-9 px of the bounds rule may legitimately flip
    W, Hh = c["image"].shape[1], c["image"].shape[0]
    with np.errstate(invalid="ignore"):
        edge = (np.abs(c["nx"]) < 1e-9) | (np.abs(c["nx"] - (W - 1)) < 1e-9) | (np.abs(c["ny"]) < 1e-9) | \
               (np.abs(c["ny"] - (Hh - 1)) < 1e-9)
    same_nan = np.isnan(out) == np.isnan(want)
    assert (same_nan | edge).all()
    m = np.isfinite(out) & np.isfinite(want)
    assert m.sum() > 100
    d = np.abs(out[m] - want[m]).max()
    print(case, "max |d| / max|image| =", d / np.nanmax(np.abs(c["image"])))
    assert d <= 1e-9 * np.nanmax(np.abs(c["image"]))
    if case != "none_m2d":  # the rotation is what is being tested: without it the result is another image
        plain = gpu_handle.resample_carrington(c["hdr"], grid, c["solar_r"], order=c["order"])
        assert not np.array_equal(plain, out, equal_nan=True)


def _align(paths, call, mode):
    from euispice_coreg_amd.hdrshift.alignment import Alignment
    ps, pl = paths
    A = Alignment(pl, ps, lag_crval1=call["lag_crval1"], lag_crval2=call["lag_crval2"], lag_cdelt1=None, lag_cdelt2=None,
                  lag_crota=call["lag_crota"], parallelism=call["parallelism"], reprojection_order=call["order"],
                  differential_rotation=mode)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = A.align_using_carrington(return_type="corr", lonlims=call["lonlims"], latlims=call["latlims"],
                                     shape=call["shape"], reference_date=call["reference_date"])
    return np.asarray(c)[:, :, 0, 0, :, 0]


ALIGNMENT_CASES = ["b174_default_date", "b304_given_date", "b304_crota_axis", "b174_parallel_order1", "outside_table",
                   "b304_argmax_moves"]


def test_every_alignment_case_is_run(alignment_golden):
    _, m, _ = alignment_golden
    assert sorted(m["cases"]) == sorted(ALIGNMENT_CASES)
    assert "b304_argmax_moves" in m["argmax_moves"]
    assert m["cases"]["outside_table"]["patched"] == m["cases"]["outside_table"]["unpatched"]


@pytest.mark.parametrize("case", ALIGNMENT_CASES)
def test_intended_alignment_matches_patched_reference(alignment_golden, case):
    _, m, paths = alignment_golden
    c = m["cases"][case]
    got = _align(paths[case], c["call"], "intended")
    want = np.asarray(c["patched"])
    assert got.shape == want.shape and np.isfinite(got).all()
    print(case, "max |d corr| =", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-10
    assert list(np.unravel_index(np.argmax(got), got.shape)) == c["argmax_patched"]


@pytest.mark.parametrize("case", ["b304_argmax_moves", "b174_default_date", "b304_crota_axis"])
def test_default_alignment_still_returns_the_unpatched_map(alignment_golden, case):
    _, m, paths = alignment_golden
    c = m["cases"][case]
    assert c["argmax_patched"] != c["argmax_unpatched"]
    got = _align(paths[case], c["call"], "reference")
    want = np.asarray(c["unpatched"])
    print(case, "max |d corr| =", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-10
    assert list(np.unravel_index(np.argmax(got), got.shape)) == c["argmax_unpatched"]


def test_jitter_session_writes_the_patched_references_cards(alignment_golden, tmp_path):
    from euispice_coreg_amd.jitter_correction import jitter_correction_imagers
    from euispice_coreg_amd.utils import fits_io
    g, m, _ = alignment_golden
    s = m["jitter"]
    paths = []
    for k, h in enumerate(s["headers"]):
        p = str(tmp_path / f"solo_L2_eui-hrieuv174-image_{k:03d}.fits")
        fits_io.write_images(p, [(None, {}), (g[f"frame{k}"], h)])
        paths.append(p)
    call = dict(s["call"])
    arrays = {k: np.asarray(call.pop(k), dtype=np.float64) for k in ("lag_crval1", "lag_crval2")}
    for mode, outputs in (("intended", s["outputs_patched"]), ("reference", s["outputs_unpatched"])):
        out = str(tmp_path / ("out_" + mode))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            jitter_correction_imagers(paths, out, differential_rotation=mode, **arrays, **call)
        for k, (p, ref) in enumerate(zip(paths, outputs)):
            _, hdr = fits_io.read_image(os.path.join(out, os.path.basename(p)), -1)
            print(mode, k, hdr["CRVAL1"] - ref["CRVAL1"], hdr["CRVAL2"] - ref["CRVAL2"])
            # the tolerances of tests/test_gpu_reference_jitter_sessions.py
            assert hdr["CROTA"] == pytest.approx(ref["CROTA"], abs=1e-12), (mode, k)
            assert abs(hdr["CRVAL1"] - ref["CRVAL1"]) < 5e-3 and abs(hdr["CRVAL2"] - ref["CRVAL2"]) < 5e-3, (mode, k, hdr["CRVAL1"], hdr["CRVAL2"], ref)
            for c in ("PC1_1", "PC1_2", "PC2_1"):
                assert hdr[c] == pytest.approx(ref[c], rel=1e-14), (mode, k, c)
    # (the two sessions differ by far more than the tolerance: the rotation is what moved the cards)
    assert abs(s["outputs_patched"][2]["CRVAL1"] - s["outputs_unpatched"][2]["CRVAL1"]) > 0.5


def _sweep(h, small, hs, large, hl, lags, shape, lonlims, latlims, rot_ref=None, rot_small=None):
    h.set_rotation("reference", rot_ref)
    h.set_rotation("small", rot_small)
    try:
        return H.gpu_carrington(h, small, hs, large, hl, lags, shape, lonlims=lonlims, latlims=latlims)
    finally:
        h.set_rotation("reference", None)
        h.set_rotation("small", None)


LAGS = (17.0 + 4.0 * (np.arange(3) - 1), -9.0 + 4.0 * (np.arange(3) - 1), None, None, [-0.3, 0.0])


def test_tile_skip_does_not_change_a_rotated_map(gpu_handle):
    """256 x 128 grid = 32 tiles of 1024 points, most of them off the image; 2 days of rotation slide the rows by up to
    a few grid steps against each other."""
    small, hs, large, hl, _ = H.scene()
    shape, lon, lat = (256, 128), (150.0, 350.0), (-80.0, 80.0)
    maps = []
    for skip in (0, 1):
        gpu_handle.set_option("tile_skip", skip)
        try:
            maps.append(_sweep(gpu_handle, small, hs, large, hl, LAGS, shape, lon, lat, ROT_304_2D, ROT_304_2D))
        finally:
            gpu_handle.set_option("tile_skip", 1)
    assert np.isfinite(maps[0]).any()
    assert np.array_equal(maps[0], maps[1], equal_nan=True)
    plain = _sweep(gpu_handle, small, hs, large, hl, LAGS, shape, lon, lat)
    assert not np.array_equal(plain, maps[0], equal_nan=True)


def test_rotation_set_then_cleared_equals_an_untouched_handle():
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene()
    shape = (72, 64)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, shape)
    with _lib.CoregHandle(0) as fresh, _lib.CoregHandle(0) as used:
        want = H.gpu_carrington(fresh, small, hs, large, hl, LAGS, shape)
        want_ref = fresh.get_reference_on_grid((64, 72), np.float64)
        want_rs = fresh.resample_carrington(hs, grid, 1.004)
        rotated = _sweep(used, small, hs, large, hl, LAGS, shape, H.CARR_LON, H.CARR_LAT, ROT_304_2D, ROT_304_2D)
        assert not np.array_equal(rotated, want, equal_nan=True)
        got = H.gpu_carrington(used, small, hs, large, hl, LAGS, shape)  # (_sweep cleared both)
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(used.get_reference_on_grid((64, 72), np.float64), want_ref, equal_nan=True)
        assert np.array_equal(used.resample_carrington(hs, grid, 1.004), want_rs, equal_nan=True)
        # a rotation over no time, or with cancelling coefficients, is the plain path too
        for rot in ((0.0, 14.51, -3.12, 0.34), (2.0, 14.18, 0.0, 0.0)):
            got = _sweep(used, small, hs, large, hl, LAGS, shape, H.CARR_LON, H.CARR_LAT, rot, rot)
            assert np.array_equal(got, want, equal_nan=True)
        with pytest.raises(_lib.CoregError):
            used.set_rotation("small", (float("nan"), 14.51, -3.12, 0.34))


def test_rotation_through_the_multi_device_driver(gpu_handle, monkeypatch):
    from euispice_coreg_amd import _lib
    monkeypatch.delenv("COREG_VIRTUAL_DEVICES", raising=False)
    small, hs, large, hl, _ = H.scene()
    shape = (72, 64)
    rot_ref, rot_small = (0.01, 14.51, -3.12, 0.34), ROT_304_2D
    want = _sweep(gpu_handle, small, hs, large, hl, LAGS, shape, H.CARR_LON, H.CARR_LAT, rot_ref, rot_small)
    plain = H.gpu_carrington(gpu_handle, small, hs, large, hl, LAGS, shape)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, shape)
    ls = _lib.LagSet(*LAGS)
    with _lib.MultiHandle(device_ids=[0]) as m:
        m.set_rotation("reference", rot_ref)
        m.set_rotation("small", rot_small)
        m.set_small(small)
        m.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        got = m.sweep_carrington(hs, grid, 1.004, ls)
        assert np.array_equal(np.asarray(got).ravel(), want.ravel(), equal_nan=True)
        m.set_rotation("reference", None)
        m.set_rotation("small", None)
        m.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        got = m.sweep_carrington(hs, grid, 1.004, ls)
        assert np.array_equal(np.asarray(got).ravel(), plain.ravel(), equal_nan=True)
    assert not np.array_equal(want, plain, equal_nan=True)
