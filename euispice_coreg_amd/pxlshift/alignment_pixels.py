"""
`AlignmentPixels` -- drop-in for euispice_coreg.pxlshift.AlignmentPixels (pxlshift/alignment_pixels.py:14-157): the
large image is brought to the small image's pixel size and the small image is slid over it in whole pixels, and
rotated about its centre, one masked Pearson coefficient per (dx, dy, drot).  The whole lag cube is one library call
(include/coreg_hip.h: coreg_pixels_sweep_method); what is not per-pixel work -- ratios, shapes, slice, bounds, the
displacement of `shift_solar_rotation_dx_large`, the checks of `method` / `min_overlap` -- is `host_plan`, numpy only and
callable without a GPU.

Beyond the reference (the defaults return what it returns): `method="residus_masked"`, the np.std of
(large - small) / sqrt(large) over the pixels finite in both images, best entry = minimum; `last_counts`, the samples
behind every entry of the last cube; `min_overlap`, entries of fewer samples set to NaN (hdrshift.alignment
.apply_min_overlap); `return_type="PixelAlignmentResults"` (pixel_alignment_results.py).

`method="mutual_information"` (not in the reference either): the mutual information, in nats, of the joint histogram of
the two images over `bins` -- the score for two instruments whose intensities are not linearly related; best entry =
maximum, the count of an entry the pairs in its histogram (`quantile_edges`, `check_edges`).

`find_local_shifts` (not in the reference either): the small image cut into tiles, one lag cube, count cube, best entry
and sub-lag fit per tile (include/coreg_hip.h: coreg_pixels_sweep_tiles; local_shift_field.py) -- the drift across a
raster whose columns were not taken at one pointing.  With `tile_step` the tiles become windows that slide by less than
their size, with `apodization` every window is weighted by a smooth bell: local correlation tracking
(coreg_pixels_sweep_windows).

Differences from the reference, all deliberate:
  * a second `find_best_parameters` call starts from the file's pixels again (the reference sub-resolves the already
    sub-resolved image);
  * a lag whose window leaves the sub-resolved image raises the reference's ValueError before any work is done (the
    reference raises it when its loop gets there);
  * an unknown `unit_rot` raises ValueError (the reference dies on an unbound name).

`smooth_large=` / `smooth_small=` (`find_best_parameters`, `find_local_shifts`; not in the reference): a NaN-aware
Gaussian smoothing of either image on the GPU, right after its pixels are set and before the solar-rotation shift and
the sub-resolution -- the anti-alias filter the order-1 point sampling of the large image lacks.  A FWHM, a pair
(fwhm_y, fwhm_x) or a pair of weight tables, in pixels of the image's own grid (utils/smoothing.py: `smoothing_tables`;
include/coreg_hip.h: coreg_pixels_smooth_large states the rule).  Default mutual-information edges are then the quantiles
of the smoothed images.

`despike_large=` / `despike_small=` (the same two calls; not in the reference): a NaN-aware median/MAD despiking of either
image on the GPU, right after its pixels are set and before the smoothing, the solar-rotation shift and the
sub-resolution.  True (the defaults), a number of sigmas or a dict (utils/despiking.py: `despike_params`;
include/coreg_hip.h: coreg_despike_small states the rule).  `self.last_despiked` = {"small": [...], "large": [...]} holds
the pixels flagged per pass.  Default mutual-information edges are the quantiles of the images as the sweep sees them:
despiked, then smoothed.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..hdrshift.alignment import apply_min_overlap, library_method, min_overlap_floor
from ..utils import fits_io, header as hdrutil, spice_header, wcs_tan
from ..utils.despiking import despike_params
from ..utils.smoothing import smoothing_tables  # noqa: F401  (the tables of `smooth_large=` / `smooth_small=`)

_RETURN_TYPES = ("corr", "PixelAlignmentResults")
MUTUAL_INFORMATION = "mutual_information"  # hdrshift's `library_method` has none: `align_using_carrington` knows it beside those
DEFAULT_BINS, MAX_BINS = 16, 32


def quantile_edges(pixels, n_bins):
    """The default edges of `n_bins` bins for an image: `np.unique` of the quantiles k / n_bins, k = 1 ... n_bins - 1, of
    its finite pixels (ties collapse to fewer bins; a constant image leaves one edge).  ValueError without a finite
    pixel."""
    v = np.asarray(pixels, dtype=np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        raise ValueError("bins: an image without a finite pixel has no quantiles")
    return np.unique(np.quantile(v, np.arange(1, n_bins) / n_bins))


def check_edges(edges, name):
    """An edge list as the library takes it: 1-D float64, 1 to 31 entries, finite, strictly increasing."""
    try:
        e = np.array(edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"bins: {name} must be a list of numbers") from None
    if e.ndim != 1 or not 1 <= e.size <= MAX_BINS - 1:
        raise ValueError(f"bins: {name} must hold 1 to {MAX_BINS - 1} edges")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError(f"bins: {name} must be finite and strictly increasing")
    return e


def zero_lag_window(large_shape, small_shape, origin, ratio1, ratio2):
    """(row slice, column slice) of the large image under the small image at lag (0, 0): rows floor(l0 ratio2) ...
    ceil((l0 + h - 1) ratio2), columns likewise with l1, w, ratio1, both ends included, clipped to the image."""
    out = []
    for n, size, l, ratio in ((large_shape[0], small_shape[0], origin[0], ratio2),
                              (large_shape[1], small_shape[1], origin[1], ratio1)):
        lo, hi = int(np.floor(l * ratio)), int(np.ceil((l + size - 1) * ratio))
        out.append(slice(max(lo, 0), min(hi, n - 1) + 1))
    return tuple(out)


def _pair_of_integers(v, name):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (rows, columns)") from None
    for x in (a, b):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"{name} must hold two integers")
    return int(a), int(b)


def tile_grid(image_shape, tile_shape, tile_step=None):
    """(th, tw), (n_ty, n_tx) of the tiles of `tile_shape` = (rows, columns) on an image of `image_shape`: whole numbers,
    1 <= th <= h, 1 <= tw <= w; the last tile of an axis is ragged when the shape does not divide it.
    tile_step = (sy, sx), 1 <= sy <= th, 1 <= sx <= tw (a larger step would leave gaps), default the tile shape: tile ty
    covers rows [ty sy, min(h, ty sy + th)), and an axis holds one tile when h <= th, else ceil((h - th) / sy) + 1 -- every
    pixel is covered, no tile lies inside its neighbour (`window_slices`)."""
    th, tw = _pair_of_integers(tile_shape, "tile_shape")
    h, w = image_shape
    if not (1 <= th <= h and 1 <= tw <= w):
        raise ValueError(f"tile_shape {(th, tw)} must lie within [1, {h}] x [1, {w}], the small image")
    if tile_step is None:
        return (th, tw), (-(-h // th), -(-w // tw))
    sy, sx = check_tile_step((th, tw), tile_step)
    return (th, tw), tuple(1 if n <= t else -(-(n - t) // s) + 1 for n, t, s in ((h, th, sy), (w, tw, sx)))


def check_tile_step(tile_shape, tile_step):
    """(sy, sx) of a `tile_step` argument: None is the tile shape; else two whole numbers within [1, th] x [1, tw]."""
    if tile_step is None:
        return int(tile_shape[0]), int(tile_shape[1])
    sy, sx = _pair_of_integers(tile_step, "tile_step")
    if not (1 <= sy <= tile_shape[0] and 1 <= sx <= tile_shape[1]):
        raise ValueError(f"tile_step {(sy, sx)} must lie within [1, {tile_shape[0]}] x [1, {tile_shape[1]}], the tile shape")
    return sy, sx


def window_slices(image_shape, tile_shape, tile_step=None):
    """[n_ty][n_tx] of (row slice, column slice): the rectangles of `tile_grid`."""
    (th, tw), (n_ty, n_tx) = tile_grid(image_shape, tile_shape, tile_step)
    sy, sx = check_tile_step((th, tw), tile_step)
    h, w = image_shape
    return [[(slice(ty * sy, min(h, ty * sy + th)), slice(tx * sx, min(w, tx * sx + tw))) for tx in range(n_tx)]
            for ty in range(n_ty)]


def gaussian_window(n, sigma):
    """The Gaussian weight table of `n` pixels about the centre (n - 1) / 2: exp(-0.5 ((r - (n - 1) / 2) / sigma)^2)."""
    r = np.arange(n, dtype=np.float64)
    return np.exp(-0.5 * ((r - (n - 1) / 2) / sigma) ** 2)


def apodization_tables(apodization, tile_shape):
    """(wy, wx), float64 tables of th and tw weights, of an `apodization` argument; None for None.  "gaussian": sigma =
    (th / 4, tw / 4); a pair of positive finite numbers: (sigma_y, sigma_x) in pixels (`gaussian_window`); a pair of 1-D
    arrays of th and tw entries, finite, >= 0, each with a positive entry: the tables themselves.  Pixel (r, c) of a
    window has the weight wy[r] * wx[c]."""
    if apodization is None:
        return None
    th, tw = tile_shape
    err = ValueError('apodization must be None, "gaussian", a pair (sigma_y, sigma_x) of positive numbers or a pair of '
                     f"tables of {th} and {tw} weights, finite, >= 0, each with a positive entry")
    if isinstance(apodization, str):
        if apodization != "gaussian":
            raise err
        apodization = (th / 4, tw / 4)
    try:
        ay, ax = apodization
        ay, ax = np.asarray(ay, dtype=np.float64), np.asarray(ax, dtype=np.float64)
    except (TypeError, ValueError):
        raise err from None
    if any(isinstance(v, (bool, np.bool_)) for v in apodization):
        raise err
    if ay.ndim == 0 and ax.ndim == 0:
        if not (np.isfinite(ay) and np.isfinite(ax) and ay > 0 and ax > 0):
            raise err
        return gaussian_window(th, float(ay)), gaussian_window(tw, float(ax))
    if ay.shape != (th,) or ax.shape != (tw,):
        raise err
    for t in (ay, ax):
        if not (np.all(np.isfinite(t)) and np.all(t >= 0) and np.any(t > 0)):
            raise err
    return np.ascontiguousarray(ay).copy(), np.ascontiguousarray(ax).copy()


def _integer_lags(v, name):
    a = np.atleast_1d(np.asarray(v))
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"{name} must be a non-empty 1-D array")
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    if a.dtype.kind == "f" and np.all(np.isfinite(a)) and np.all(a == np.rint(a)):
        return a.astype(np.int64)
    raise TypeError(f"{name}: slice indices must be integers")


class AlignmentPixels:

    def __init__(self, large_fov_known_pointing, window_large, small_fov_to_correct, window_small, device=None):
        data, hdr = fits_io.read_image(large_fov_known_pointing, window_large)
        self.hdr_large = fits_io.Header(hdr).copy()
        self.data_large = np.array(fits_io.native_pixels(data), dtype=np.float64)
        data, hdr = fits_io.read_image(small_fov_to_correct, window_small)
        self.hdr_small = fits_io.Header(hdr).copy()
        self.data_small = np.array(fits_io.native_pixels(data), dtype=np.float64)
        self.large_fov_known_pointing, self.window_large = large_fov_known_pointing, window_large
        self.small_fov_to_correct, self.window_small = small_fov_to_correct, window_small
        self.device = device
        self.slc_small_ref = None
        self.ratio_res_1 = self.ratio_res_2 = None
        self.last_timing = None
        self.last_counts = None
        self.last_despiked = None  # {"small": [...], "large": [...]}: pixels flagged per pass in the last call

    # ------------------------------------------------------------------------------------------------------------
    def _return_shift_large_fov_solar_rotation(self):
        """alignment_pixels.py:109-124: apparent solar rotation between the two exposures [arcsec]."""
        hl = self.hdr_large
        band = hl["WAVELNTH"]
        B0 = np.deg2rad(hl["SOLAR_B0"])
        omega_car = np.deg2rad(360 / 25.38 / 86400)
        if band == 174:
            band = 171
        omega = omega_car + spice_header.diff_rot(B0, f"EIT {band}")
        Rsun, Dsun = hl["RSUN_REF"], hl["DSUN_OBS"]
        phi = np.rad2deg(omega * Rsun / (Dsun - Rsun)) * 3600
        # (astropy's Time difference: whole days and day fractions apart, then to seconds)
        day_s, frac_s = spice_header._mjd_parts(self.hdr_small["DATE-AVG"])
        day_l, frac_l = spice_header._mjd_parts(hl["DATE-AVG"])
        dt = ((day_s - day_l) + (frac_s - frac_l)) * 86400.0
        return dt * phi

    def _shift_large_fov_displacement(self):
        """alignment_pixels.py:91-99: (dx, dy) in pixels of the large image."""
        hl = self.hdr_large
        dcrval = self._return_shift_large_fov_solar_rotation()
        d1 = float(hdrutil.convert(dcrval, "arcsec", hl["CUNIT1"]))
        if "CROTA" in hl:
            theta = np.deg2rad(hl["CROTA"])
            d2 = float(hdrutil.convert(dcrval, "arcsec", hl["CUNIT2"]))
            return float((d1 / hl["CDELT1"]) * np.cos(-theta)), float((d2 / hl["CDELT2"]) * np.sin(-theta))
        return float(d1 / hl["CDELT1"]), 0.0

    def host_plan(self, lag_dx, lag_dy, lag_drot, unit_rot="degree", shift_solar_rotation_dx_large=False,
                  method="correlation", min_overlap=None, tile_shape=None, bins=None, tile_step=None,
                  apodization=None, smooth_large=None, smooth_small=None, despike_large=None, despike_small=None) -> dict:
        """Everything of a `find_best_parameters` call that is decided on the host (numpy only, no GPU); with
        `tile_shape` = (rows, columns), of a `find_local_shifts` call: the plan then holds the tile grid too.
        `bins` (method "mutual_information" only, ValueError with any other): an integer 2 <= B <= 32 (default 16) --
        `quantile_edges` of the small image and of the large image's pixels under the zero-lag window
        (`zero_lag_window`), so the edges do not depend on the lags -- or a pair (edges_small, edges_large) as
        `check_edges` takes them; the plan holds the pair as `plan["bins"]`.
        `tile_step` (with `tile_shape`; `tile_grid`): the plan holds it next to the shape and the grid.  `apodization` (with
        `tile_shape`, method "correlation" only, ValueError with any other; `apodization_tables`): the plan holds the two
        weight tables as `plan["window"]` = (wy, wx), None without.  `smooth_large`, `smooth_small` (`smoothing_tables`, in
        pixels of each image's own grid): the plan holds the table pairs under those names, None without; with either,
        `bins` as a number cannot be turned into edges here -- they are quantiles of the smoothed images, which the GPU
        makes -- and the plan holds the number as `plan["bins_pending"]` and `plan["bins"]` = None until the call has them.
        `despike_large`, `despike_small` (`despike_params`): held under those names as dicts, None without; what is said of
        `bins` with a smoothing holds with a despiking too."""
        smooth = {"smooth_large": smoothing_tables(smooth_large, "smooth_large"),
                  "smooth_small": smoothing_tables(smooth_small, "smooth_small"),
                  "despike_large": despike_params(despike_large, "despike_large"),
                  "despike_small": despike_params(despike_small, "despike_small")}
        if method == MUTUAL_INFORMATION:
            method_code = _lib.METHOD_MUTUAL_INFORMATION
        else:
            method_code = library_method(method)
            if bins is not None:
                raise ValueError("bins belongs to method='mutual_information'")
        if method_code == _lib.METHOD_RESIDUS:
            raise NotImplementedError("pxlshift has no unmasked 'residus' (the reference's pxlshift has no such score): "
                                      "use 'residus_masked'")
        if min_overlap is not None:
            min_overlap_floor(min_overlap)  # (a fraction is taken of the sweep's largest count, once that is known)
        dx, dy = _integer_lags(lag_dx, "lag_dx"), _integer_lags(lag_dy, "lag_dy")
        drot = np.atleast_1d(np.asarray(lag_drot, dtype=np.float64))
        if drot.ndim != 1 or drot.size == 0:
            raise ValueError("lag_drot must be a non-empty 1-D array")
        if unit_rot == "degree":
            drot_rad = np.radians(drot)
        elif unit_rot == "radian":
            drot_rad = drot.copy()
        else:
            raise ValueError("unit_rot must be 'degree' or 'radian'")
        hs, hl = self.hdr_small, self.hdr_large
        ratio1 = float(hdrutil.convert(hs["CDELT1"], hs["CUNIT1"], hl["CUNIT1"])) / hl["CDELT1"]
        ratio2 = float(hdrutil.convert(hs["CDELT2"], hs["CUNIT2"], hl["CUNIT2"])) / hl["CDELT2"]
        if not (ratio1 > 0 and ratio2 > 0):
            raise ValueError("the pixel sizes of the two images must have the same sign")
        H, W = self.data_large.shape
        h, w = self.data_small.shape
        sub = (len(np.arange(0, H, ratio2)), len(np.arange(0, W, ratio1)))
        l = [int((sub[n] - (h, w)[n] - 1) / 2) for n in range(2)]
        # alignment_pixels.py:150-156, for every lag
        if (l[0] + dy.min() < 0 or l[0] + h + dy.max() > sub[0] or l[1] + dx.min() < 0 or l[1] + w + dx.max() > sub[1]):
            raise ValueError("too large shift : outside FSI")
        plan = {"lag_dx": dx, "lag_dy": dy, "lag_drot": drot, "lag_drot_rad": drot_rad, "unit_rot": unit_rot,
                "ratio_res_1": float(ratio1), "ratio_res_2": float(ratio2), "sub_shape": sub, "slc_small_ref": tuple(l),
                "xc": round(w / 2), "yc": round(h / 2), "shift_large": None, "method": method,
                "method_code": method_code, "min_overlap": min_overlap, "small_shape": (h, w), **smooth}
        if method == MUTUAL_INFORMATION:
            bins = DEFAULT_BINS if bins is None else bins
            if (isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_))
                    and any(v is not None for v in smooth.values())):
                if not 2 <= bins <= MAX_BINS:
                    raise ValueError(f"bins as a number must lie in [2, {MAX_BINS}]")
                plan["bins"], plan["bins_pending"] = None, int(bins)
            else:
                plan["bins"] = self._bin_edges(bins, plan)
        if tile_shape is None:
            if tile_step is not None or apodization is not None:
                raise ValueError("tile_step and apodization belong to a tile_shape")
        else:
            plan["tile_shape"], plan["tile_grid"] = tile_grid((h, w), tile_shape, tile_step)
            plan["tile_step"] = check_tile_step(plan["tile_shape"], tile_step)
            if apodization is not None and method != "correlation":
                raise ValueError("apodization belongs to method='correlation' (no weighted residus_masked or histogram)")
            plan["window"] = apodization_tables(apodization, plan["tile_shape"])
        if shift_solar_rotation_dx_large:
            plan["shift_large"] = self._shift_large_fov_displacement()
        return plan

    def _bin_edges(self, bins, plan, small=None, large=None):
        """(edges_small, edges_large) of a `bins` argument (see `host_plan`); `small`, `large`: the images a number of
        bins is the quantiles of (default: the file's pixels)."""
        if isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_)):
            if not 2 <= bins <= MAX_BINS:
                raise ValueError(f"bins as a number must lie in [2, {MAX_BINS}]")
            small = self.data_small if small is None else small
            large = self.data_large if large is None else large
            win = zero_lag_window(self.data_large.shape, self.data_small.shape, plan["slc_small_ref"],
                                  plan["ratio_res_1"], plan["ratio_res_2"])
            return quantile_edges(small, int(bins)), quantile_edges(large[win], int(bins))
        if isinstance(bins, (bool, np.bool_, float, np.floating, str)):
            raise ValueError("bins must be an integer or a pair (edges_small, edges_large)")
        try:
            es, el = bins
        except (TypeError, ValueError):
            raise ValueError("bins must be an integer or a pair (edges_small, edges_large)") from None
        return check_edges(es, "edges_small"), check_edges(el, "edges_large")

    def _set_images(self, hnd, plan):
        """Every call starts from the file's pixels: both images up, despiked and then smoothed where the plan says so
        (and the pending default bins taken from them), then the solar-rotation shift of the large one."""
        hnd.pixels_set_large(self.data_large)
        hnd.pixels_set_small(self.data_small)
        self.last_despiked = {"small": [], "large": []}
        if plan["despike_large"] is not None:
            self.last_despiked["large"] = hnd.pixels_despike_large(plan["despike_large"])
        if plan["despike_small"] is not None:
            self.last_despiked["small"] = hnd.pixels_despike_small(plan["despike_small"])
        if plan["smooth_large"] is not None:
            hnd.pixels_smooth_large(plan["smooth_large"])
        if plan["smooth_small"] is not None:
            hnd.pixels_smooth_small(plan["smooth_small"])
        if plan.get("bins_pending") is not None:
            large = (None if plan["smooth_large"] is None and plan["despike_large"] is None
                     else hnd.pixels_get_image("large", self.data_large.shape))
            small = (None if plan["smooth_small"] is None and plan["despike_small"] is None
                     else hnd.pixels_get_image("small", self.data_small.shape))
            plan["bins"] = self._bin_edges(plan["bins_pending"], plan, small, large)
        if plan["shift_large"] is not None:
            dx, dy = plan["shift_large"]
            hnd.pixels_shift_large(dx, dy)
            print(f"corrected solar rotation on FSI on CRVAL1: {dx=}, {dy=}")

    def find_best_parameters(self, lag_dx, lag_dy, lag_drot, unit_rot="degree", shift_solar_rotation_dx_large=False,
                             method="correlation", min_overlap=None, return_type="corr", bins=None, smooth_large=None,
                             smooth_small=None, despike_large=None, despike_small=None):
        """alignment_pixels.py:57-84: correlation cube [len(lag_dx), len(lag_dy), len(lag_drot)], float64.
        method: "correlation" (best = maximum), "residus_masked" (best = minimum) or "mutual_information" (best =
        maximum; `bins` as `host_plan` takes it).  `self.last_counts`: the samples
        behind every entry, shaped like the cube (before `min_overlap`).  min_overlap: None, a count >= 1 or a fraction
        in (0, 1) of the sweep's largest count; entries of fewer samples become NaN, ValueError when none is left.
        return_type: "corr" (the cube) or "PixelAlignmentResults".  smooth_large, smooth_small, despike_large,
        despike_small: see the module docstring."""
        if return_type not in _RETURN_TYPES:
            raise ValueError(f"return_type must be one of {_RETURN_TYPES}")
        plan = self.host_plan(lag_dx, lag_dy, lag_drot, unit_rot, shift_solar_rotation_dx_large, method, min_overlap,
                              bins=bins, smooth_large=smooth_large, smooth_small=smooth_small, despike_large=despike_large,
                              despike_small=despike_small)
        self.lag_dx, self.lag_dy, self.lag_drot, self.unit_rot = lag_dx, lag_dy, lag_drot, unit_rot
        self.ratio_res_1, self.ratio_res_2 = plan["ratio_res_1"], plan["ratio_res_2"]
        l, (h, w) = plan["slc_small_ref"], self.data_small.shape
        self.slc_small_ref = (slice(l[0], l[0] + h), slice(l[1], l[1] + w))
        hnd = _lib.shared_handle(-1 if self.device is None else self.device)
        self._set_images(hnd, plan)
        corr = hnd.pixels_sweep(plan, plan["method_code"])
        self.last_timing = hnd.pixels_last_timing()
        self.last_counts = hnd.pixels_last_counts(corr.shape)
        self._last_plan = plan
        corr = apply_min_overlap(corr, self.last_counts, min_overlap)
        if return_type == "corr":
            return corr
        from .pixel_alignment_results import PixelAlignmentResults
        return PixelAlignmentResults(corr, plan["lag_dx"], plan["lag_dy"], plan["lag_drot"], unit_rot=unit_rot,
                                     method=method, n_samples=self.last_counts,
                                     large_fov_path=self.large_fov_known_pointing, large_fov_window=self.window_large,
                                     small_fov_path=self.small_fov_to_correct)

    def find_local_shifts(self, lag_dx, lag_dy, lag_drot=(0.0,), tile_shape=None, unit_rot="degree",
                          shift_solar_rotation_dx_large=False, method="correlation", min_overlap=None, min_fill=0.5,
                          sub_lag=True, bins=None, tile_step=None, apodization=None, smooth_large=None, smooth_small=None,
                          despike_large=None, despike_small=None):
        """The local shift field: the small image is cut into tiles of `tile_shape` = (rows, columns) pixels (the last
        ones ragged) and every tile gets the lag cube of `find_best_parameters` on its own rectangle -- a rotated plane
        is still rotated about the whole image's centre -- with its sample counts, best entry and sub-lag fit.  Returns a
        `LocalShiftField` (local_shift_field.py), which takes `min_overlap` (per tile), `min_fill` and `sub_lag`.

        tile_step = (sy, sx), 1 <= sy <= th, 1 <= sx <= tw: windows that slide by less than their size (`tile_grid`); the
        default, the tile shape, is the disjoint tiles.  apodization (method "correlation" only): None, "gaussian" (sigma
        = (th / 4, tw / 4)), (sigma_y, sigma_x) in pixels, or two tables of th and tw weights (`apodization_tables`):
        pixel (r, c) of a window weighs wy[r] * wx[c] in the means and the three sums of its coefficient; a ragged
        window uses the head of the tables (a bell cut off about the nominal centre; its `tile_centres` entry stays
        the centre of the clipped rectangle).  The count of an entry stays the kept pixels, whatever their weight; the sum
        of their weights is the field's `weight_sums`, and `min_fill` then compares weights, not pixels."""
        if tile_shape is None:
            raise ValueError("tile_shape = (rows, columns) is needed")
        plan = self.host_plan(lag_dx, lag_dy, lag_drot, unit_rot, shift_solar_rotation_dx_large, method, min_overlap,
                              tile_shape=tile_shape, bins=bins, tile_step=tile_step, apodization=apodization,
                              smooth_large=smooth_large, smooth_small=smooth_small, despike_large=despike_large,
                              despike_small=despike_small)
        hnd = _lib.shared_handle(-1 if self.device is None else self.device)
        self._set_images(hnd, plan)
        corr = hnd.pixels_sweep_tiles(plan, plan["method_code"])
        self.last_timing = hnd.pixels_last_timing()
        counts = hnd.pixels_last_tile_counts(corr.shape)
        weights = None if plan["window"] is None else hnd.pixels_last_tile_weights(corr.shape)
        self._last_plan = plan
        from .local_shift_field import LocalShiftField
        return LocalShiftField(corr, counts, plan["lag_dx"], plan["lag_dy"], plan["lag_drot"], plan["tile_shape"],
                               self.data_small.shape, unit_rot=unit_rot, method=method, min_overlap=min_overlap,
                               min_fill=min_fill, sub_lag=sub_lag, tile_step=plan["tile_step"], weight_sums=weights,
                               window=plan["window"])

    # read-backs of the last call's device images (tests, inspection)
    def _large_box(self):
        p = self._last_plan
        h, w = self.data_small.shape
        shape = (h + int(p["lag_dy"].max() - p["lag_dy"].min()), w + int(p["lag_dx"].max() - p["lag_dx"].min()))
        return _lib.shared_handle(-1 if self.device is None else self.device).pixels_get_large_box(shape)

    def _rotated(self, k):
        return _lib.shared_handle(-1 if self.device is None else self.device).pixels_get_rotated(k, self.data_small.shape)


def align_pixels_shift(delta_pix1, delta_pix2, windows, large_fov_fits_path, large_fov_window, small_fov_path):
    """Util.AlignCommonUtil.align_pixels_shift (utils/Util.py:248-278): the header of the small image's window with
    CRVAL at the large image's centre plus (delta_pix1, delta_pix2) of its own pixels, CRPIX at its own centre.  As the
    reference, it returns the header of the last window of `windows`."""
    mid = large_fov_centre(large_fov_fits_path, large_fov_window)
    out = None
    for win in windows:
        out = fits_io.Header(fits_io.read_header(small_fov_path, win)).copy()
        set_pixels_shift_cards(out, mid, delta_pix1, delta_pix2)
    return out


def large_fov_centre(large_fov_fits_path, large_fov_window):
    """(longitude, latitude) [deg] of the centre of the large image's window (utils/Util.py:254-262)."""
    header_fsi = fits_io.Header(fits_io.read_header(large_fov_fits_path, large_fov_window))
    w_fsi = wcs_tan.TanWcs(header_fsi)
    naxis1, naxis2 = w_fsi.naxis
    lon_mid, lat_mid = w_fsi.pixel_to_world(np.array([(naxis1 - 1) / 2]), np.array([(naxis2 - 1) / 2]))
    return lon_mid[0], lat_mid[0]


def set_pixels_shift_cards(out, mid, delta_pix1, delta_pix2):
    """The four cards `align_pixels_shift` sets, in place (utils/Util.py:266-276)."""
    n1 = out["ZNAXIS1"] if "ZNAXIS1" in out else out["NAXIS1"]
    n2 = out["ZNAXIS2"] if "ZNAXIS2" in out else out["NAXIS2"]
    out["CRVAL1"] = float(hdrutil.convert(mid[0], "deg", out["CUNIT1"])) + delta_pix1 * out["CDELT1"]
    out["CRVAL2"] = float(hdrutil.convert(mid[1], "deg", out["CUNIT2"])) + delta_pix2 * out["CDELT2"]
    out["CRPIX1"] = (n1 + 1) / 2
    out["CRPIX2"] = (n2 + 1) / 2
