#!/opt/conda/bin/python3.9
"""
Golden-vector generator (reference) for the pixel-lag alignment: the REFERENCE's own `AlignmentPixels`
(`pxlshift/alignment_pixels.py`) and `AlignmentSpicePixel` (`pxlshift/alignment_spice_pixel.py`), loaded through
`_reference_loader` (numba's `jit` is the identity there: `pxlshift/c_correlate.py:41-63` runs as plain numpy), and
`Util.AlignCommonUtil.align_pixels_shift` (`utils/Util.py:248-278`).

    tests/golden/pxlshift_golden.npz    inputs (float32-exact pixels), correlation cubes, sub-resolved boxes, rotated
                                        planes, shifted images, the prepared SPICE image
    tests/golden/pxlshift_golden.json   headers, lags, ratios, shapes, slices, printed (dx, dy), consumed header cards

Cases:
  a  25 x 21 in 80 x 96, ratios 0.9 / 0.8, 7 x 5 x {0, 1.5, -2.0} deg; NaN pixels in both images
  b  70 x 130 in 200 x 260, ratios 1.3 / 0.7, 19 x 17 x {0, 0.02 rad}, unit_rot='radian'
  c  a's images, lags that reach the edges of the sub-resolved image exactly; one lag further raises
  d  a's shapes, 3 x 3 x {0}, shift_solar_rotation_dx_large=True with and without CROTA
  e  AlignmentSpicePixel on synthetic.make_spice_l2(nx=24, ny=80, nw=6, large_n=128)
  f  a flat small image (all-NaN cube); one lag out of bounds (ValueError)

The generator refuses to write unless the comparison is fair: no rotated coordinate within 1e-6 px of 0 or n - 1 (a
sample decided there by libm noise flips between NaN and a value), and the best entry of every cube leads the second
best by more than 4 * 2^-23 (the argmax is not decided by the float32 rounding of the numerator).

Run (build container only; a few seconds):
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_pxlshift.py
"""
import contextlib
import importlib.util
import io
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _reference_loader  # noqa: E402

_reference_loader.load_reference()

import numpy as np  # noqa: E402
import scipy.ndimage  # noqa: E402
from astropy.io import fits  # noqa: E402
from euispice_coreg.pxlshift.alignment_pixels import AlignmentPixels  # noqa: E402
from euispice_coreg.pxlshift.alignment_spice_pixel import AlignmentSpicePixel  # noqa: E402
from euispice_coreg.utils import matrix_transform  # noqa: E402
from euispice_coreg.utils import Util  # noqa: E402

spec = importlib.util.spec_from_file_location("coreg_synthetic", os.path.join(ROOT, "euispice_coreg_amd", "synthetic.py"))
synthetic = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synthetic)

ARR, META = {}, {"cases": {}}
STRUCTURAL = {"SIMPLE", "BITPIX", "EXTEND", "XTENSION", "PCOUNT", "GCOUNT", "END", "COMMENT", "HISTORY", ""}


def plain(v):
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if isinstance(v, np.ndarray):
        return [plain(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def cards(h):
    return {k: plain(h[k]) for k in h.keys() if k not in STRUCTURAL and not k.startswith("NAXIS")}


def to_header(d):
    h = fits.Header()
    for k, v in d.items():
        if not k.startswith("NAXIS"):
            h[k] = v
    return h


def blob_field(rng, shape, n_blobs):
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    img = np.full(shape, 100.0)
    for _ in range(n_blobs):
        cx, cy = rng.uniform(0, shape[1]), rng.uniform(0, shape[0])
        s, a = rng.uniform(1.5, 7.0), np.exp(rng.uniform(np.log(50.0), np.log(2000.0)))
        img += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return img


def make_pair(seed, small_shape, large_shape, cdelt_large, cdelt_small, offset, nan_small=0.0, nan_large=0.0):
    """A large image and a small one cut from its sub-resolved version `offset` = (dx, dy) pixels off the centred
    slice, with its own gain and noise; float32-exact float64 pixels (as FITS BITPIX=-32 data cast to float64)."""
    rng = np.random.default_rng(seed)
    large = blob_field(rng, large_shape, max(12, large_shape[0] * large_shape[1] // 400))
    large = large + np.sqrt(large) * rng.standard_normal(large.shape)
    large = large.astype(np.float32).astype(np.float64)
    r1, r2 = cdelt_small[0] / cdelt_large[0], cdelt_small[1] / cdelt_large[1]
    x, y = np.meshgrid(np.arange(0, large_shape[1], r1), np.arange(0, large_shape[0], r2))
    sub = scipy.ndimage.map_coordinates(large, np.stack((y.ravel(), x.ravel())), order=1, mode="constant", cval=0.0,
                                        prefilter=False).reshape(x.shape)
    h, w = small_shape
    l0, l1 = int((sub.shape[0] - h - 1) / 2), int((sub.shape[1] - w - 1) / 2)
    small = 0.7 * sub[l0 + offset[1]:l0 + offset[1] + h, l1 + offset[0]:l1 + offset[0] + w] + 30.0
    small = small + 0.5 * np.sqrt(small) * rng.standard_normal(small.shape)
    small = small.astype(np.float32).astype(np.float64)
    if nan_small > 0:
        small[rng.random(small.shape) < nan_small] = np.nan
    if nan_large > 0:
        large[rng.random(large.shape) < nan_large] = np.nan
    hl = {"CTYPE1": "HPLN-TAN", "CTYPE2": "HPLT-TAN", "CUNIT1": "arcsec", "CUNIT2": "arcsec",
          "CRPIX1": (large_shape[1] + 1) / 2.0, "CRPIX2": (large_shape[0] + 1) / 2.0, "CRVAL1": -300.0, "CRVAL2": 400.0,
          "CDELT1": float(cdelt_large[0]), "CDELT2": float(cdelt_large[1]), "WAVELNTH": 174, "SOLAR_B0": -3.1,
          "RSUN_REF": 695700000.0, "DSUN_OBS": 0.38 * synthetic.AU, "DATE-AVG": "2022-03-17T09:50:45.281"}
    hs = {"CTYPE1": "HPLN-TAN", "CTYPE2": "HPLT-TAN", "CUNIT1": "arcsec", "CUNIT2": "arcsec",
          "CRPIX1": (w + 1) / 2.0, "CRPIX2": (h + 1) / 2.0, "CRVAL1": -300.0, "CRVAL2": 400.0,
          "CDELT1": float(cdelt_small[0]), "CDELT2": float(cdelt_small[1]), "DATE-AVG": "2022-03-17T10:15:45.281"}
    return small, hs, large, hl


def write_pair(tmp, name, small, hs, large, hl):
    p_large = os.path.join(tmp, name + "_large.fits")
    p_small = os.path.join(tmp, name + "_small.fits")
    fits.HDUList([fits.PrimaryHDU(data=large, header=to_header(hl))]).writeto(p_large, overwrite=True)
    fits.HDUList([fits.PrimaryHDU(data=small, header=to_header(hs))]).writeto(p_small, overwrite=True)
    return p_large, p_small


def f32_exact(a):
    b = np.asarray(a, dtype=np.float32)
    assert np.array_equal(b.astype(np.float64), a, equal_nan=True)
    return b


def check_gap(name, corr):
    v = np.sort(corr[np.isfinite(corr)])[::-1]
    assert v.size >= 2 and v[0] - v[1] > 4 * 2.0 ** -23, (name, "argmax decided by the float32 rounding", v[:2])


def check_rotated_coordinates(name, shape, lag_drot, unit_rot):
    xx, yy = np.meshgrid(np.arange(shape[1]), np.arange(shape[0]))
    for drot in lag_drot:
        if drot == 0:
            continue
        nx, ny = matrix_transform.MatrixTransform.polar_transform(xx, yy, theta=drot, units=unit_rot)
        for c, n in ((nx, shape[1]), (ny, shape[0])):
            d = np.minimum(np.abs(c), np.abs(c - (n - 1)))
            assert d.min() > 1e-6, (name, "a rotated coordinate lies within 1e-6 px of the image edge", drot, d.min())


def run(A, lag_dx, lag_dy, lag_drot, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        corr = A.find_best_parameters(np.asarray(lag_dx), np.asarray(lag_dy), np.asarray(lag_drot), **kw)
    return np.asarray(corr, dtype=np.float64), out.getvalue()


def record(name, A, corr, lag_dx, lag_dy, lag_drot, unit_rot, extra=None, rotated=True):
    h, w = A.data_small.shape
    l0, l1 = A.slc_small_ref[0].start, A.slc_small_ref[1].start
    assert A.slc_small_ref[0].stop == l0 + h and A.slc_small_ref[1].stop == l1 + w
    ARR[f"{name}/corr"] = corr
    # the part of the sub-resolved image the sweep can read
    ARR[f"{name}/large_box"] = np.array(A.data_large[l0 + min(lag_dy):l0 + h + max(lag_dy),
                                                     l1 + min(lag_dx):l1 + w + max(lag_dx)], dtype=np.float64)
    entry = {"lag_dx": plain(lag_dx), "lag_dy": plain(lag_dy), "lag_drot": plain(lag_drot), "unit_rot": unit_rot,
             "ratio_res_1": float(A.ratio_res_1), "ratio_res_2": float(A.ratio_res_2),
             "ratio_res_1_hex": float(A.ratio_res_1).hex(), "ratio_res_2_hex": float(A.ratio_res_2).hex(),
             "sub_shape": list(A.data_large.shape), "slc_small_ref": [l0, l1], "shape": list(corr.shape)}
    if rotated and lag_drot[-1] != 0:
        ARR[f"{name}/data_small_rotated"] = np.array(A.data_small_rotated, dtype=np.float64)
        entry["rotated_index"] = len(lag_drot) - 1
    entry.update(extra or {})
    META["cases"][name] = entry
    fin = np.isfinite(corr)
    print(f"{name:14s} corr {corr.shape} nan {int((~fin).sum())} argmax "
          f"{np.unravel_index(np.nanargmax(corr), corr.shape) if fin.any() else None} "
          f"max {np.nanmax(corr) if fin.any() else None}", flush=True)


def main():
    tmp = tempfile.mkdtemp(prefix="golden_pxlshift_")

    # ------------------------------------------------------------------------------------------------------- case a
    small, hs, large, hl = make_pair(101, (25, 21), (80, 96), (4.0, 4.0), (3.6, 3.2), (1, -1), 0.03, 0.01)
    ARR["a/small"], ARR["a/large"] = f32_exact(small), f32_exact(large)
    META["hdr_a_small"], META["hdr_a_large"] = hs, hl
    pl, ps = write_pair(tmp, "a", small, hs, large, hl)
    ldx, ldy, lrot = list(range(-3, 4)), list(range(-2, 3)), [0.0, 1.5, -2.0]
    check_rotated_coordinates("a", small.shape, lrot, "degree")
    A = AlignmentPixels(pl, 0, ps, 0)
    corr, _ = run(A, ldx, ldy, lrot)
    assert A.ratio_res_1 == 0.9 and A.ratio_res_2 == 0.8
    check_gap("a", corr)
    record("a", A, corr, ldx, ldy, lrot, "degree")

    # ------------------------------------------------------------------------------------------------------- case c
    A = AlignmentPixels(pl, 0, ps, 0)
    sub = (len(np.arange(0, 80, 0.8)), len(np.arange(0, 96, 0.9)))
    l0, l1 = int((sub[0] - 25 - 1) / 2), int((sub[1] - 21 - 1) / 2)
    ldx_c = [-l1, -20, 0, 1, 22, sub[1] - 21 - l1]
    ldy_c = [-l0, -1, 0, sub[0] - 25 - l0]
    corr, _ = run(A, ldx_c, ldy_c, [0.0])
    assert tuple(A.data_large.shape) == sub and A.slc_small_ref[0].start == l0 and A.slc_small_ref[1].start == l1
    check_gap("c", corr)
    beyond = []
    for bdx, bdy in (([ldx_c[0] - 1], [0]), ([ldx_c[-1] + 1], [0]), ([0], [ldy_c[0] - 1]), ([0], [ldy_c[-1] + 1])):
        B = AlignmentPixels(pl, 0, ps, 0)
        try:
            run(B, bdx, bdy, [0.0])
            raise AssertionError("one lag beyond the edge did not raise")
        except ValueError as e:
            beyond.append({"lag_dx": bdx, "lag_dy": bdy, "raises": "ValueError", "message": str(e)})
    record("c", A, corr, ldx_c, ldy_c, [0.0], "degree", {"inputs": "a", "beyond": beyond})

    # ------------------------------------------------------------------------------------------------------- case b
    small, hs, large, hl = make_pair(202, (70, 130), (200, 260), (4.0, 4.0), (5.2, 2.8), (-2, 3), 0.01, 0.002)
    ARR["b/small"], ARR["b/large"] = f32_exact(small), f32_exact(large)
    META["hdr_b_small"], META["hdr_b_large"] = hs, hl
    pl, ps = write_pair(tmp, "b", small, hs, large, hl)
    ldx, ldy, lrot = list(range(-9, 10)), list(range(-8, 9)), [0.0, 0.02]
    check_rotated_coordinates("b", small.shape, lrot, "radian")
    A = AlignmentPixels(pl, 0, ps, 0)
    corr, _ = run(A, ldx, ldy, lrot, unit_rot="radian")
    assert corr.size == 646
    check_gap("b", corr)
    record("b", A, corr, ldx, ldy, lrot, "radian")

    # ------------------------------------------------------------------------------------------------------- case d
    small, hs, large, hl = make_pair(303, (25, 21), (80, 96), (4.0, 4.0), (3.6, 3.2), (3, 0), 0.02, 0.01)
    ARR["d/small"], ARR["d/large"] = f32_exact(small), f32_exact(large)
    for tag, crota in (("d_crota", 5.0), ("d_nocrota", None)):
        hl_d = dict(hl)
        if crota is not None:
            hl_d["CROTA"] = crota
        META[f"hdr_{tag}_small"], META[f"hdr_{tag}_large"] = hs, hl_d
        pl, ps = write_pair(tmp, tag, small, hs, large, hl_d)
        S = AlignmentPixels(pl, 0, ps, 0)
        with contextlib.redirect_stdout(io.StringIO()):
            S._shift_large_fov()
        ARR[f"{tag}/shifted"] = np.array(S.data_large, dtype=np.float64)
        A = AlignmentPixels(pl, 0, ps, 0)
        ldx = ldy = [-1, 0, 1]
        corr, printed = run(A, ldx, ldy, [0.0], shift_solar_rotation_dx_large=True)
        m = re.search(r"dx=([-+0-9.eE]+), dy=([-+0-9.eE]+)", printed)
        assert m, printed
        check_gap(tag, corr)
        record(tag, A, corr, ldx, ldy, [0.0], "degree",
               {"inputs": "d", "printed_dx": float(m.group(1)), "printed_dy": float(m.group(2))})

    # ------------------------------------------------------------------------------------------------------- case e
    cube, h4, large, hl, truth = synthetic.make_spice_l2(nx=24, ny=80, nw=6, large_n=128, pointing_error=(3.0, -2.0, 0.0))
    large32 = np.asarray(large, dtype=np.float32)
    ARR["e/cube"], ARR["e/large"] = cube, large32
    p_spice = os.path.join(tmp, "solo_L2_spice-n-ras_20220317T094045_V01.fits")
    p_fsi = os.path.join(tmp, "solo_L2_eui-fsi174-image_ref.fits")
    fits.HDUList([fits.PrimaryHDU(data=cube, header=to_header(h4))]).writeto(p_spice, overwrite=True)
    fits.HDUList([fits.PrimaryHDU(), fits.ImageHDU(data=large32, header=to_header(hl))]).writeto(p_fsi, overwrite=True)
    with fits.open(p_spice) as f:
        META["hdr_e_spice"] = cards(f[0].header)
    with fits.open(p_fsi) as f:
        META["hdr_e_fsi"] = cards(f[1].header)
    with contextlib.redirect_stdout(io.StringIO()):
        A = AlignmentSpicePixel(p_fsi, 1, p_spice, 0)
    assert A.data_small.shape == (62, 24), A.data_small.shape
    ARR["e/data_small"] = np.array(A.data_small, dtype=np.float64)
    consumed = {k: plain(A.hdr_small[k]) for k in ("CDELT1", "CDELT2", "CUNIT1", "CUNIT2", "DATE-AVG")}
    ldx, ldy = list(range(-7, 3)), list(range(11, 26))
    corr, _ = run(A, ldx, ldy, [0.0])
    check_gap("e", corr)
    i, j, _k = np.unravel_index(np.nanargmax(corr), corr.shape)
    assert 0 < i < len(ldx) - 1 and 0 < j < len(ldy) - 1, ("the lag range does not contain the peak", i, j)
    extra = {"file_spice": os.path.basename(p_spice), "file_fsi": os.path.basename(p_fsi), "fsi_window": 1,
             "spice_window": 0, "hdr_small_consumed": consumed}
    # the one consumer of the result: best (dx, dy) -> header (Util.py:248-278)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            hdr = Util.AlignCommonUtil.align_pixels_shift(float(ldx[i]), float(ldy[j]), [0], p_fsi, 1, p_spice)
        extra["align_pixels_shift"] = {"delta_pix1": float(ldx[i]), "delta_pix2": float(ldy[j]), "windows": [0],
                                       "header": {k: plain(hdr[k]) for k in ("CRVAL1", "CRVAL2", "CRPIX1", "CRPIX2")}}
    except Exception as e:  # recorded, not hidden
        extra["align_pixels_shift"] = {"raises": type(e).__name__, "message": str(e)[:300]}
        print("align_pixels_shift raises", type(e).__name__, str(e)[:200], flush=True)
    record("e", A, corr, ldx, ldy, [0.0], "degree", extra)

    # ------------------------------------------------------------------------------------------------------- case f
    small = np.full((25, 21), 7.0)
    pl, ps = write_pair(tmp, "f", small, META["hdr_a_small"], ARR["a/large"].astype(np.float64), META["hdr_a_large"])
    A = AlignmentPixels(pl, 0, ps, 0)
    with np.errstate(all="ignore"):
        corr, _ = run(A, [-1, 0, 1], [0, 1], [0.0])
    assert np.isnan(corr).all()
    ARR["f/corr"] = corr
    META["cases"]["f"] = {"inputs_large": "a", "small_value": 7.0, "small_shape": [25, 21], "lag_dx": [-1, 0, 1],
                          "lag_dy": [0, 1], "lag_drot": [0.0], "shape": list(corr.shape),
                          "out_of_bounds": {"lag_dx": [0, 60], "lag_dy": [0], "raises": "ValueError"}}
    B = AlignmentPixels(pl, 0, ps, 0)
    try:
        run(B, [0, 60], [0], [0.0])
        raise AssertionError("an out-of-bounds lag did not raise")
    except ValueError as e:
        META["cases"]["f"]["out_of_bounds"]["message"] = str(e)

    import astropy
    import scipy
    META["interpreter"] = {"python": sys.version.split()[0], "numpy": np.__version__, "scipy": scipy.__version__,
                           "astropy": astropy.__version__}
    dst = os.path.join(HERE, "pxlshift_golden.npz")
    np.savez_compressed(dst, **ARR)
    with open(os.path.join(HERE, "pxlshift_golden.json"), "w") as f:
        json.dump(META, f, indent=1, sort_keys=True)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
