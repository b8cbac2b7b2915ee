#!/opt/conda/bin/python3.9
"""
Golden-vector generator: the REFERENCE's own `utils/rectify.py` with its differential rotation switched ON --
`CarringtonTransform(hdr, reference_date=..., rate_wave=band)` + `Rectifier` -- on the 64 x 64 images and small grids of
`make_golden_rectify.py`.  The reference's `Alignment` never gets here (its band lookup fails, quirk Q5); the transform
itself is complete, and `differential_rotation="intended"` is pinned to it.

Run (build container only; /root/reference must exist):
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_rectify_diffrot.py

Per case: the inputs, `x1` = the rotated longitudes `transform_1(x, y)[0]` (float64, so that dx = x - x1 up to the
rounding of that subtraction), `dx` = `-transform_1(0, y)[0]` (the shift itself, exact: 0 - dx), `nx`, `ny`, the resampled
image and astropy's `delta_t`; `x` and `dx` as the one row / one column they repeat.  Only the reference module is executed; nothing of it is copied.
"""
import importlib.util
import os
import sys

import numpy as np

for _n, _v in [("asscalar", lambda a: a.item()), ("alen", len)]:
    if not hasattr(np, _n):
        setattr(np, _n, _v)
np._set_promotion_state("weak")

REF = "/root/reference/euispice_coreg/utils/rectify.py"
spec = importlib.util.spec_from_file_location("ref_rectify", REF)
rectify = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rectify)

AU = 1.495978707e11
DATE_OBS = "2022-03-17T09:50:45.277"
# reference dates that put DATE-OBS at -2 d, +10 min and +0.15 d (3 h 36 min)
REF_DATES = {"m2d": "2022-03-19T09:50:45.277", "p10min": "2022-03-17T09:40:45.277", "p015d": "2022-03-17T06:14:45.277"}


def make_image(rng, ny, nx, nan_frac):
    yy, xx = np.mgrid[0:ny, 0:nx]
    img = 100.0 + 50.0 * np.sin(xx / 5.3) * np.cos(yy / 7.1) + 30.0 * rng.standard_normal((ny, nx))
    img += 400.0 * np.exp(-((xx - nx * 0.4) ** 2 + (yy - ny * 0.6) ** 2) / (2 * 6.0 ** 2))
    img[rng.random((ny, nx)) < nan_frac] = np.nan
    return img


def run_case(name, hdr, band, when, solar_r, shape, lonlims, latlims, order, img, out):
    t = rectify.CarringtonTransform(hdr, radius_correction=solar_r, reference_date=REF_DATES[when], rate_wave=band)
    r = rectify.Rectifier(t)
    res = r(img, shape, lonlims, latlims, order=order, fill=-32762)
    x, y = r.coordinates
    assert x.dtype == np.float32 and y.dtype == np.float32
    x1 = t.transform_1(x=x, y=y)[0]
    dx = -t.transform_1(x=np.zeros_like(x), y=y)[0]
    nx, ny = t(x=x, y=y)
    assert nx.dtype == np.float64 and x1.dtype == np.float64 and dx.dtype == np.float64
    res = np.where(res == -32762, np.nan, res)
    keys = ["CROTA", "CROTA2", "CRVAL1", "CRVAL2", "CRPIX1", "CRPIX2", "CDELT1", "CDELT2", "DSUN_OBS", "CRLN_OBS",
            "CRLT_OBS"]
    out[name + "/hdr_keys"] = np.array([k for k in keys if k in hdr])
    out[name + "/hdr_vals"] = np.array([float(hdr[k]) for k in keys if k in hdr])
    out[name + "/date_obs"] = np.array(hdr["DATE-OBS"])
    out[name + "/reference_date"] = np.array(REF_DATES[when])
    out[name + "/band"] = np.array(str(band))  # "None": outside the table
    out[name + "/coeffs"] = np.array(t.transform_1.coeffs, dtype=np.float64)
    out[name + "/delta_t"] = np.float64(t.transform_1.delta_t)
    out[name + "/solar_r"] = np.float64(solar_r)
    out[name + "/shape"] = np.array(shape)
    out[name + "/lonlims"] = np.array(lonlims, dtype=np.float64)
    out[name + "/latlims"] = np.array(latlims, dtype=np.float64)
    out[name + "/order"] = np.int64(order)
    out[name + "/image"] = img
    assert np.array_equal(x, np.broadcast_to(x[:1], x.shape)) and np.array_equal(dx, np.broadcast_to(dx[:, :1], dx.shape))
    out[name + "/x"] = x[0]       # [n_lon] float32: the grid's longitudes (every row the same)
    out[name + "/x1"] = x1
    out[name + "/dx"] = dx[:, 0]  # [n_lat]: every column the same
    out[name + "/nx"] = nx
    out[name + "/ny"] = ny
    out[name + "/resampled"] = res
    print(name, "band", band, "delta_t", float(t.transform_1.delta_t), "max|dx| deg", np.abs(dx).max(), "grid",
          res.shape, "finite", np.isfinite(res).sum(), "of", res.size)


def main():
    rng = np.random.default_rng(20220318)
    out = {}
    base = {"CROTA": 3.0, "CRVAL1": -310.0, "CRVAL2": 420.0, "CRPIX1": 32.5, "CRPIX2": 32.5, "CDELT1": 15.7,
            "CDELT2": 15.7, "DSUN_OBS": 0.38 * AU, "CRLN_OBS": 250.0, "CRLT_OBS": -3.0, "DATE-OBS": DATE_OBS}
    wide = dict(base)  # rotated, anisotropic CDELT, the whole disc in the field of view
    wide.update({"CROTA": 31.7, "CDELT1": 40.0, "CDELT2": 27.0, "CRVAL1": 55.5, "CRVAL2": -120.25, "CRPIX1": 30.0,
                 "CRPIX2": 35.0, "DSUN_OBS": 0.61 * AU})
    img = make_image(rng, 64, 64, 0.01)
    img_wide = make_image(rng, 64, 64, 0.0)
    # every band once; delta_t of -2 d, +10 min, +0.15 d; orders 1 and 2
    run_case("b171_p015d", dict(base), "171", "p015d", 1.004, [48, 40], [228.0, 262.0], [-12.0, 22.0], 2, img, out)
    run_case("b195_m2d", dict(base), "195", "m2d", 1.004, [64, 64], [230.0, 260.0], [-10.0, 20.0], 2, img, out)
    run_case("b304_p10min_o1", dict(base), "304", "p10min", 1.004, [33, 47], [236.0, 256.0], [-4.0, 16.0], 1, img, out)
    # grid reaching beyond the limb (zz < 0 -> NaN), latitudes to +-85 deg
    run_case("b284_m2d_limb", dict(wide), "284", "m2d", 1.0, [56, 24], [120.0, 380.0], [-85.0, 85.0], 2, img_wide, out)
    # |lat| > 60 deg throughout the upper half: the sin^2 / sin^4 terms carry the shift
    run_case("b304_p015d_highlat", dict(wide), "304", "p015d", 1.0, [40, 48], [200.0, 300.0], [35.0, 82.0], 2, img_wide,
             out)
    run_case("b171_m2d_highlat_o1", dict(wide), "171", "m2d", 1.0, [40, 48], [200.0, 300.0], [-82.0, -35.0], 1, img_wide,
             out)
    # CROTA2 keyword instead of CROTA, non-square image, shifted header (a "lag")
    hd = dict(base)
    del hd["CROTA"]
    hd["CROTA2"] = -12.25
    hd["CRVAL1"] += 17.0
    hd["CRVAL2"] -= 9.0
    hd["CRPIX1"] = 40.5
    run_case("b171_m2d_crota2", hd, "171", "m2d", 1.004, [40, 40], [235.0, 258.0], [-6.0, 18.0], 2,
             make_image(rng, 48, 80, 0.02), out)
    # a band outside the transform's table: coefficients (14.18, 0, 0), dx == 0 exactly
    run_case("none_m2d", dict(base), None, "m2d", 1.004, [48, 40], [228.0, 262.0], [-12.0, 22.0], 2, img, out)

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rectify_diffrot_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; numpy", np.__version__, "python", sys.version.split()[0])


if __name__ == "__main__":
    main()
