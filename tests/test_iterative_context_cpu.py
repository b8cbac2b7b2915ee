"""CPU tests of the iterative-context SPICE alignment (`AlignementSpiceIterativeContextRaster`,
include/coreg_hip.h: coreg_sweep_context): the C ABI, the constructor, the frame of every raster column, the per-lag
header planning against wcslib's own arithmetic, and the reference-run fixture (tests/golden/iterative_context_golden;
generator tests/golden/make_golden_iterative_context.py) replayed through a NumPy / SciPy restatement of the
reference's `_step` kept in this file."""
import ctypes as C
import inspect
import json
import os
import re
import warnings

import numpy as np
import pytest

from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster  # noqa: F401  (the feature under test)
from tests.conftest import GOLDEN
from tests.test_reference_spice_fuzz_cpu import inputs
from tests.test_reference_spice_fuzz_cpu import load as load_spice
from tests.test_reference_synras_fuzz_cpu import load as load_synras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load():
    g = np.load(os.path.join(GOLDEN, "iterative_context_golden.npz"))
    with open(os.path.join(GOLDEN, "iterative_context_golden.json")) as f:
        return g, json.load(f)


def cases():
    with open(os.path.join(GOLDEN, "iterative_context_golden.json")) as f:
        return sorted(json.load(f)["cases"])


def scene(name, tmp_path, frame_dtype=np.float64, compressed=False):
    """The SPICE file and imager sequence of window `name` of synras_fuzz_golden, written as FITS files:
    (spice path, imager paths, synras case)."""
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.utils import fits_io
    gs, ms = load_spice()
    _, mr = load_synras()[:2]
    sp = ms["scenes"]
    c = mr["cases"][name]
    cube, h4, large, hl = inputs(gs, ms, name)
    p_spice = str(tmp_path / sp[name]["file"])
    fits_io.write_images(p_spice, [(cube, h4)])
    frames = synthetic.make_imager_sequence(large.astype(np.float64), hl, start=c["start"], cadence_s=c["cadence_s"],
                                            n_frames=c["n_frames"])
    paths = []
    for j, (img, _) in enumerate(frames):
        p = str(tmp_path / f"solo_L2_eui-fsi174-image_{j:02d}.fits")
        hdr = dict(c["imager_headers"][j])
        img = np.asarray(img, dtype=frame_dtype)
        if compressed:  # Rice tiles of the float32 pixels (quantised)
            fits_io.write_compressed_image(p, img.astype(np.float32), hdr, quantize="NO_DITHER")
        else:
            fits_io.write_images(p, [(None, {}), (img, hdr)])
        paths.append(p)
    return p_spice, paths, c


def make(case, p_spice, paths, **kw):
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster
    lags = [None if v is None else np.asarray(v, dtype=np.float64) for v in case["lags_arcsec"]]
    return AlignementSpiceIterativeContextRaster(
        large_fov_list_paths=paths, small_fov_to_correct=p_spice, threshold_time=case["threshold_time"],
        lag_crval1=lags[0], lag_crval2=lags[1], lag_cdelt1=lags[2], lag_cdelt2=lags[3], lag_crota=lags[4],
        small_fov_value_min=case["small_fov_value_min"], small_fov_value_max=case["small_fov_value_max"],
        small_fov_window=0, cdelt_semantics="reference", **kw)


# ---- the C ABI ---------------------------------------------------------------------------------------------------
NEW = ["coreg_set_context_frames", "coreg_context_frame_from_small", "coreg_sweep_context", "coreg_context_lag_headers"]


def test_new_symbols_are_exported_with_the_header_s_arity():
    from euispice_coreg_amd import _lib
    lib = _lib.load_library()
    text = open(os.path.join(ROOT, "include", "coreg_hip.h")).read()
    table = {n: a for n, _, a in _lib.SYMBOLS}
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(table[name]), name


def test_struct_layouts_match_the_header():
    from euispice_coreg_amd import _lib
    # coreg_wcs2d: 2 int32 + 17 double + 2 int32 (include/coreg_hip.h), coreg_lags: 5 x (pointer, int32)
    assert C.sizeof(_lib.Wcs2d) == 8 + 17 * 8 + 8
    assert _lib.Wcs2d.proj.offset == 8 + 17 * 8
    assert C.sizeof(_lib.Lags) == 5 * 16


# ---- the public class ----------------------------------------------------------------------------------------------
# the reference's constructor (alignment_spice.py:358-362), keyword for keyword
REFERENCE_INIT = ["large_fov_list_paths", "small_fov_to_correct", "threshold_time", "lag_crval1", "lag_crval2",
                  "lag_cdelt1", "lag_cdelt2", "lag_crota", "small_fov_value_min", "parallelism", "small_fov_value_max",
                  "counts_cpu_max", "large_fov_window", "small_fov_window", "use_tqdm", "path_save_figure"]
REFERENCE_DEFAULTS = {"small_fov_value_min": None, "parallelism": False, "small_fov_value_max": None,
                      "counts_cpu_max": 40, "large_fov_window": -1, "small_fov_window": -1, "use_tqdm": False,
                      "path_save_figure": None}


def test_class_signature_matches_the_reference():
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster as A
    params = list(inspect.signature(A.__init__).parameters.values())[1:]
    assert [p.name for p in params[:len(REFERENCE_INIT)]] == REFERENCE_INIT
    for p in params[:len(REFERENCE_INIT)]:
        if p.name in REFERENCE_DEFAULTS:
            assert p.default == REFERENCE_DEFAULTS[p.name], p.name
        else:
            assert p.default is inspect.Parameter.empty, p.name
    assert all(p.default is not inspect.Parameter.empty for p in params[len(REFERENCE_INIT):])
    sig = inspect.signature(A.align_using_helioprojective)
    assert list(sig.parameters) == ["self", "method", "index_amplitude", "extend_pixel_size"]


@pytest.mark.parametrize("name", ["P00", "P05"])
def test_frame_of_every_column_is_the_map_builder_s(name, tmp_path):
    """The frame of every column, against SPICEComposedMapBuilder's own choice (synras_fuzz_golden: what the
    reference's builder took for this window and sequence)."""
    from euispice_coreg_amd.utils import fits_io
    _, mr = load_synras()[:2]
    p_spice, paths, c = scene(name, tmp_path)
    A = make({"lags_arcsec": [None] * 5, "threshold_time": c["threshold_time"], "small_fov_value_min": None,
              "small_fov_value_max": None}, p_spice, paths)
    h4 = fits_io.Header(fits_io.read_header(p_spice, 0))
    got = A._frame_of_columns(h4, [fits_io.read_header(p, -1) for p in paths])
    assert got.tolist() == mr["cases"][name]["frame_of_column"]


def test_threshold_time_raises(tmp_path):
    from euispice_coreg_amd.utils import fits_io
    p_spice, paths, c = scene("P05", tmp_path)
    A = make({"lags_arcsec": [None] * 5, "threshold_time": 1.0, "small_fov_value_min": None,
              "small_fov_value_max": None}, p_spice, paths)
    h4 = fits_io.Header(fits_io.read_header(p_spice, 0))
    with pytest.raises(ValueError, match="sufficiently close in time"):
        A._frame_of_columns(h4, [fits_io.read_header(p, -1) for p in paths[:1]])


def test_level_3_is_refused():
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster as A
    a = A(["x.fits"], "solo_L3_spice.fits", 60.0, [0.0], [0.0], None, None, None)
    with pytest.raises(NotImplementedError):
        a.align_using_helioprojective()


# ---- per-lag planning ------------------------------------------------------------------------------------------------
def prepared(name, tmp_path, lags):
    """(AlignmentSpice-prepared class, 4-D celestial target, imager headers, frame of every column)"""
    from euispice_coreg_amd.utils import fits_io, header as hdrutil
    p_spice, paths, c = scene(name, tmp_path)
    A = make({"lags_arcsec": lags, "threshold_time": c["threshold_time"], "small_fov_value_min": None,
              "small_fov_value_max": None}, p_spice, paths)
    A.extend_pixel_size = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        A._extract_spice_data_header(level=2, coeff=None)
        A._set_initial_header_values(True)
    headers = []
    for p in paths:
        hw = fits_io.Header(fits_io.read_header(p, -1))
        hdrutil.check_and_create_pcij_matrix(hw, False, warn=False)
        headers.append(hw)
    cf = A._frame_of_columns(A.header_spice_unflattened, headers)
    return A, A._celestial_degrees(A.header_spice_unflattened, A.hdr_small), headers, cf


def test_lag_homographies_agree_with_wcslib(tmp_path):
    from euispice_coreg_amd import _lib
    A, target, headers, cf = prepared("P00", tmp_path, [[-4.0, 0.0, 6.0], [3.0], None, [0.1], [0.0, 0.7]])
    ny, nx = int(A.hdr_small["NAXIS2"]), int(A.hdr_small["NAXIS1"])
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    for d in [(A.lag_crval1[0], A.lag_crval2[0], 0.0, 0.0, 0.0), (A.lag_crval1[2], A.lag_crval2[0], 0.0,
                                                                   A.lag_cdelt2[0], A.lag_crota[1])]:
        ctx, grid, shifted = _lib.context_lag_headers(target, A.hdr_small, *d)
        hc, hg, hs = (_lib.wcs_to_dict(w) for w in (ctx, grid, shifted))
        # the SPICE resample: near identity, the exact homography within 1e-9 px of wcslib's chain
        ox, oy, _, _ = _lib.wcslib_pixel_to_pixel(hg, hs, xx, yy)
        H = np.array(_lib.homography(hg, hs)).reshape(3, 3)
        w = H[2, 0] * xx + H[2, 1] * yy + H[2, 2]
        assert np.abs((H[0, 0] * xx + H[0, 1] * yy + H[0, 2]) / w - ox.reshape(xx.shape)).max() < 1e-9
        assert np.abs((H[1, 0] * xx + H[1, 1] * yy + H[1, 2]) / w - oy.reshape(xx.shape)).max() < 1e-9
        assert np.abs(ox.reshape(xx.shape) - xx).max() < 1e-6
        # the context: slit pixels of the shifted 4-D grid -> the pixels of the frame each column takes
        for f in sorted(set(cf.tolist()))[:4]:
            ox, oy, _, _ = _lib.wcslib_pixel_to_pixel(hc, headers[f], xx, yy)
            H = np.array(_lib.homography(hc, headers[f])).reshape(3, 3)
            w = H[2, 0] * xx + H[2, 1] * yy + H[2, 2]
            assert np.abs((H[0, 0] * xx + H[0, 1] * yy + H[0, 2]) / w - ox.reshape(xx.shape)).max() < 1e-8
            assert np.abs((H[1, 0] * xx + H[1, 1] * yy + H[1, 2]) / w - oy.reshape(xx.shape)).max() < 1e-8


def test_grid_header_is_printed_with_14_digits(tmp_path):
    from euispice_coreg_amd import _lib
    A, target, _, _ = prepared("P05", tmp_path, [[2.0], [0.0], None, None, None])
    _, grid, shifted = _lib.context_lag_headers(target, A.hdr_small, A.lag_crval1[0], 0.0, 0.0, 0.0, 0.0)
    assert grid.crval1 == float("%.14G" % (A.hdr_small["CRVAL1"] + A.lag_crval1[0]))
    assert shifted.crval1 == float("%.16G" % (A.hdr_small["CRVAL1"] + A.lag_crval1[0]))
    assert grid.cdelt1 == A.hdr_small["CDELT1"] and grid.pc1_2 == A.hdr_small["PC1_2"]


# ---- the fixture, replayed ------------------------------------------------------------------------------------------
def replay(A, target, headers, cf, method):
    """The reference's `_step` restated with NumPy / SciPy for every lag-point: context composed column by column
    (order-2 interpol2d of the frame of that column at wcslib's coordinates of the shifted slit pixels), SPICE image
    resampled at wcslib's coordinates of the composed grid (float32 destination), thresholds, mask, c_correlate /
    residus."""
    from scipy.ndimage import map_coordinates
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.utils import fits_io
    ny, nx = int(A.hdr_small["NAXIS2"]), int(A.hdr_small["NAXIS1"])
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    frames = {f: np.asarray(fits_io.read_image(A.large_fov_list_paths[f], -1)[0], dtype=np.float64)
              for f in set(cf.tolist())}
    L = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in
         (A.lag_crval1, A.lag_crval2, A.lag_cdelt1, A.lag_cdelt2, A.lag_crota)]
    out = np.full([len(v) for v in L], np.nan)
    small = np.asarray(A.data_small, dtype=np.float64)
    for idx in np.ndindex(out.shape):
        r = _lib.context_lag_headers(target, A.hdr_small, *[L[k][idx[k]] for k in range(5)],
                                     cdelt_semantics=_lib.CDELT_REFERENCE)
        if r is None:
            continue
        hc, hg, hs = (_lib.wcs_to_dict(w) for w in r)
        large = np.empty((ny, nx))
        for f, img in frames.items():
            cols = np.nonzero(cf == f)[0]
            ox, oy, _, _ = _lib.wcslib_pixel_to_pixel(hc, headers[f], xx[:, cols], yy[:, cols])
            large[:, cols] = map_coordinates(img, np.stack((oy, ox)), order=2, mode="constant", cval=np.nan,
                                             prefilter=False).reshape(ny, len(cols))
        ox, oy, _, _ = _lib.wcslib_pixel_to_pixel(hg, hs, xx, yy)
        b = map_coordinates(small, np.stack((oy, ox)), order=2, mode="constant", cval=np.nan, prefilter=False)
        b = b.astype(np.float32).astype(np.float64)
        a = large.ravel()
        sel = np.ones(a.size, dtype=bool)
        bf = b.astype(np.float32)
        if A.small_fov_value_min is not None:
            sel &= bf > np.float32(A.small_fov_value_min)
        if A.small_fov_value_max is not None:
            sel &= bf < np.float32(A.small_fov_value_max)
        if method == "residus":
            with np.errstate(all="ignore"):
                out[idx] = np.std(((a - b) / np.sqrt(a))[sel]) if sel.any() else np.nan
            continue
        m = sel & ~np.isnan(a) & ~np.isnan(b)
        A_, B_ = a[m], b[m]
        with np.errstate(all="ignore"):
            da, db = A_ - A_.mean(), B_ - B_.mean()
            out[idx] = np.sum(da * db) / np.sqrt(np.sum(da * da) * np.sum(db * db))
    return out


@pytest.mark.parametrize("cname", cases())
def test_fixture_replayed_by_the_numpy_restatement(cname, tmp_path):
    g, m = load()
    case = m["cases"][cname]
    A, target, headers, cf = prepared(case["window"], tmp_path, case["lags_arcsec"])
    A.small_fov_value_min, A.small_fov_value_max = case["small_fov_value_min"], case["small_fov_value_max"]
    got = replay(A, target, headers, cf, case["method"])
    want = g[f"{cname}/corr"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-7, np.nanmax(np.abs(got - want))
