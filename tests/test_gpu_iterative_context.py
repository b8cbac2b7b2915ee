"""GPU tests of the iterative-context SPICE alignment (`AlignementSpiceIterativeContextRaster`, one fused sweep,
csrc/kernels_context.hpp) against the reference-run fixture (tests/golden/iterative_context_golden; generator
tests/golden/make_golden_iterative_context.py), against the per-lag composition through the library's existing calls,
and across lag slices and frame storage."""
import warnings

import numpy as np
import pytest

from tests.test_iterative_context_cpu import cases, load, make, prepared, scene

pytestmark = pytest.mark.gpu


def run(case, p_spice, paths, **kw):
    A = make(case, p_spice, paths, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = A.align_using_helioprojective(method=case["method"])
    return A, res


@pytest.mark.parametrize("cname", cases())
def test_matches_the_reference_run(cname, tmp_path):
    g, m = load()
    case = m["cases"][cname]
    p_spice, paths, _ = scene(case["window"], tmp_path)
    A, res = run(case, p_spice, paths)
    got = np.asarray(res.corr)[..., 0]
    want = g[f"{cname}/corr"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-7, np.nanmax(np.abs(got - want))
    if case["method"] == "correlation":
        assert np.nanargmax(got) == np.nanargmax(want)
    else:
        assert np.nanargmin(got) == np.nanargmin(want)


def per_lag_composition(A, target, headers, cf, vmin=None):
    """The same sweep through the library's existing calls, lag by lag: the context composed with
    resample_helioprojective per frame (what SPICEComposedMapBuilder.process_from_header does), the SPICE image
    resampled onto it (its border samples as wcslib decides them), Pearson in NumPy."""
    from scipy.ndimage import map_coordinates
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.utils import fits_io
    h = _lib.shared_handle(-1)
    h.reference_tag = None
    ny, nx = int(A.hdr_small["NAXIS2"]), int(A.hdr_small["NAXIS1"])
    L = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in
         (A.lag_crval1, A.lag_crval2, A.lag_cdelt1, A.lag_cdelt2, A.lag_crota)]
    frames = {f: fits_io.read_image(A.large_fov_list_paths[f], -1)[0] for f in set(cf.tolist())}
    out = np.full([len(v) for v in L], np.nan)
    for idx in np.ndindex(out.shape):
        r = _lib.context_lag_headers(target, A.hdr_small, *[L[k][idx[k]] for k in range(5)],
                                     cdelt_semantics=_lib.CDELT_REFERENCE)
        hc, hg, hs = (_lib.wcs_to_dict(w) for w in r)
        large = np.empty((ny, nx))
        for f, img in frames.items():
            h.set_small(img)
            cols = np.nonzero(cf == f)[0]
            large[:, cols] = h.resample_helioprojective(hc, headers[f], order=2,
                                                        dtype=np.float32 if img.dtype == np.float32 else np.float64)[:, cols]
        small = np.asarray(A.data_small, dtype=np.float64)
        h.set_small(small)
        b = h.resample_helioprojective(hg, hs, order=2, dtype=np.float32).astype(np.float64)
        # the border samples of this near-identity map sit within wcslib's rounding noise of the image's bounds: they
        # are kept or dropped as wcslib's coordinates say (alignment.py:1038-1069), sampled there
        edge = np.zeros((ny, nx), dtype=bool)
        edge[:, [0, -1]] = True
        edge[[0, -1], :] = True
        ey, ex = np.nonzero(edge)
        ox, oy, _, _ = _lib.wcslib_pixel_to_pixel(hg, hs, ex.astype(np.float64), ey.astype(np.float64))
        inside = (ox >= 0) & (ox <= nx - 1) & (oy >= 0) & (oy <= ny - 1)
        vals = map_coordinates(small, np.stack((oy, ox)), order=2, mode="constant", cval=np.nan, prefilter=False)
        b[ey, ex] = np.where(inside, vals.astype(np.float32).astype(np.float64), np.nan)
        b = b.ravel()
        a = large.ravel()
        m = ~np.isnan(a) & ~np.isnan(b)
        if vmin is not None:
            m &= b.astype(np.float32) > np.float32(vmin)
        A_, B_ = a[m], b[m]
        da, db = A_ - A_.mean(), B_ - B_.mean()
        out[idx] = np.sum(da * db) / np.sqrt(np.sum(da * da) * np.sum(db * db))
    return out


def test_fused_sweep_equals_the_per_lag_composition(tmp_path):
    lags = [[-6.0, -2.0, 0.0, 3.0, 7.5], [-3.0, 0.0, 4.5], None, None, [0.0, 0.4]]
    A, target, headers, cf = prepared("P00", tmp_path, lags)
    case = {"lags_arcsec": lags, "threshold_time": A.threshold_time, "small_fov_value_min": None,
            "small_fov_value_max": None, "method": "correlation"}
    _, res = run(case, A.small_fov_to_correct, A.large_fov_list_paths)
    got = np.asarray(res.corr)[..., 0]
    want = per_lag_composition(A, target, headers, cf)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-10, np.nanmax(np.abs(got - want))


def test_lag_slices_concatenate_to_the_whole_sweep(tmp_path):
    from euispice_coreg_amd import _lib
    lags = [[-4.0, 0.0, 4.0, 8.0], [-2.0, 2.0, 6.0], None, None, [0.0, 0.3]]
    A, target, headers, cf = prepared("P05", tmp_path, lags)
    h = _lib.shared_handle(-1)
    h.reference_tag = None
    from euispice_coreg_amd.utils import fits_io
    used = sorted(set(cf.tolist()))
    h.set_context_frames([fits_io.read_image(A.large_fov_list_paths[f], -1)[0] for f in used],
                         [headers[f] for f in used])
    h.set_small(np.asarray(A.data_small, dtype=np.float64))
    ls = _lib.LagSet(A.lag_crval1, A.lag_crval2, A.lag_cdelt1, A.lag_cdelt2, A.lag_crota)
    col = np.searchsorted(np.asarray(used), cf)
    whole = h.sweep_context(target, A.hdr_small, col, ls, vmin=60.0)
    parts = [h.sweep_context(target, A.hdr_small, col, ls, vmin=60.0, lag_begin=b, lag_end=e)
             for b, e in ((0, 5), (5, 6), (6, 17), (17, ls.size))]
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)
    import torch
    dev = torch.full((ls.size,), 7.0, dtype=torch.float64, device="cuda")
    h.sweep_context(target, A.hdr_small, col, ls, vmin=60.0, out_dev_ptr=dev.data_ptr())
    assert np.array_equal(dev.cpu().numpy(), whole, equal_nan=True)


def test_frame_storage_float32_float64_and_rice(tmp_path):
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.utils import fits_io
    g, m = load()
    case = m["cases"]["P05_crval_min"]
    maps = {}
    for kind, kw in (("f64", dict(frame_dtype=np.float64)), ("f32", dict(frame_dtype=np.float32)),
                     ("rice", dict(frame_dtype=np.float32, compressed=True))):
        d = tmp_path / kind
        d.mkdir()
        p_spice, paths, _ = scene(case["window"], d, **kw)
        A, res = run(case, p_spice, paths)
        maps[kind] = np.asarray(res.corr)
        if kind == "rice":
            # the GPU's decode of the Rice tiles against the host's: the same frames uploaded as decoded pixels
            A2 = make(case, p_spice, paths)
            A2.raw_fits_upload = False
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                maps["rice_host"] = np.asarray(A2.align_using_helioprojective(method=case["method"]).corr)
            assert isinstance(fits_io.load_for_upload(paths[0], -1)[0], fits_io.CompressedImage)
    assert np.array_equal(maps["rice"], maps["rice_host"], equal_nan=True)
    assert np.array_equal(maps["f32"], maps["rice"], equal_nan=True) or \
        np.nanmax(np.abs(maps["f32"] - maps["rice"])) < 1e-3  # (quantised tiles)
    assert np.nanmax(np.abs(maps["f32"] - maps["f64"])) < 1e-6
    assert np.nanargmax(maps["f32"]) == np.nanargmax(maps["f64"])
    want = g["P05_crval_min/corr"][..., None]
    assert np.nanmax(np.abs(maps["f64"] - want)) <= 1e-7
    del _lib


def test_write_corrected_fits_on_the_result(tmp_path):
    from euispice_coreg_amd.utils import fits_io
    g, m = load()
    case = m["cases"]["P00_crval"]
    p_spice, paths, _ = scene(case["window"], tmp_path)
    _, res = run(case, p_spice, paths)
    out = str(tmp_path / "corrected.fits")
    res.write_corrected_fits(window_list_to_apply_shift=[0], path_to_l3_output=out)
    hdr = fits_io.read_header(out, 0)
    h4 = fits_io.read_header(p_spice, 0)
    # the pointing moved by an amount inside the lag grid, the rest of the header is the input's
    for k, lag in ((1, case["lags_arcsec"][0]), (2, case["lags_arcsec"][1])):
        d = hdr[f"CRVAL{k}"] - h4[f"CRVAL{k}"]
        assert min(lag) - 1e-6 <= d <= max(lag) + 1e-6, (k, d)
    assert hdr["NAXIS1"] == h4["NAXIS1"] and hdr["CDELT1"] == h4["CDELT1"]


def test_a_combination_range_is_refused_and_does_not_outlive_the_context_sweep():
    """combo_begin / combo_end (the one-shot combination range of a grid-shared sweep) do not apply to the context
    sweep: it refuses them and takes them off the handle, so the next helioprojective sweep covers every lag."""
    from euispice_coreg_amd import _lib
    from tests import context_cases as CC
    from tests import helpers as H
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=112)
    lags = (2.0 * (np.arange(5) - 2), 2.0 * (np.arange(4) - 2), None, None, [0.0, 0.5])
    with _lib.CoregHandle(0) as fresh:
        want = H.gpu_helio(fresh, small, hs, large, hl, lags)
    with _lib.CoregHandle(0) as h:
        h.set_option("combo_begin", 0)
        h.set_option("combo_end", 1)
        with pytest.raises(_lib.CoregError) as e:
            CC.gpu(h, CC.make_case(0))
        assert e.value.code == _lib.COREG_EINVAL
        got = H.gpu_helio(h, small, hs, large, hl, lags)
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
