"""
`Alignment` -- drop-in for euispice_coreg.hdrshift.Alignment (hdrshift/alignment.py:45-399) whose lag sweep
(`_find_best_header_parameters`, alignment.py:613-797) runs on MI355X through libcoreg_hip.so.

Same constructor keywords, same `align_using_helioprojective()` / `align_using_carrington()` signatures, same
6-D correlation array layout [crval1, crval2, cdelt1, cdelt2, crota, solar_r] and the same `AlignmentResults`
surface.  Differences, all deliberate and listed in DESIGN.md:
  * `parallelism` no longer chooses between a process pool and a Python loop: both values run on the GPU.  It keeps
    its *numerical* meaning for the helioprojective frame: True = reference image resampled once
    on the small image's own pixel grid, float32 (alignment.py:649-651); False = correlate on the full large-FOV
    grid, float64 reference (alignment.py:765).
  * `counts_cpu_max`, `display_progress_bar`, `path_save_figure` are accepted and ignored.
  * CDELT lags follow the intended semantics of utils/Util.py:199-215 (quirk Q2) unless
    `cdelt_semantics="reference"`.
  * `differential_rotation="intended"` rotates both Carrington resamples to `reference_date` (utils/diffrot.py); the
    default "reference" ignores the date, as the reference's failed band lookup makes it do (quirk Q5).
  * inputs may be FITS paths or (data, header) pairs; astropy is optional.
  * with torch.distributed initialised (one process per GPU) the lag grid is sharded and all-gathered
    (euispice_coreg_amd/parallel.py); without it, `parallelism=True` drives every visible GPU from this one process
    (include/coreg_hip.h: coreg_multi) -- the unchanged user script uses the whole node, as it does with the reference.
  * `method="residus_masked"` (every `align_using_*`): the residus over the co-finite grid points only, best entry =
    the MINIMUM (quirk Q8: the reference's `residus` forgets its NaN mask and is NaN on any practical grid; it stays
    so).  After a sweep `self.last_counts` holds the per-lag sample counts (6-D like the map); `min_overlap` (an
    integer count, or a fraction in (0, 1) of the sweep's largest count) turns lag-points with fewer samples into NaN.
  * `align_using_carrington(method="mutual_information", bins=...)`: the mutual information (nats) of the joint histogram
    of the reference on the Carrington grid and the resampled image to align over `bins`, best entry = the MAXIMUM -- for
    two instruments whose intensities are not linearly related (include/coreg_hip.h: coreg_sweep_set_bins states the rule).
    The Carrington frame only: the other `align_using_*` raise NotImplementedError for it.  `self.last_bins` holds the
    edges used.
  * `smooth_small=` / `smooth_large=` (every `align_using_*`, every method): a NaN-aware Gaussian smoothing of the image to
    align (after its thresholds) and of the reference image (before its once-only resample) on the GPU, to bring the finer
    image to the coarser one's resolution (include/coreg_hip.h: coreg_smooth_small states the rule).  A FWHM, a pair
    (fwhm_y, fwhm_x) or a pair of weight tables (utils/smoothing.py: `smoothing_tables`), in pixels of each image's own grid
    or, `smooth_unit="arcsec"`, converted with each image's own CDELT.  A non-finite pixel stays NaN and gives nothing to
    its neighbours.  None (the default) changes nothing.
  * `despike_small=` / `despike_large=` (every `align_using_*`, every method): a NaN-aware median/MAD despiking of the
    image to align (after its thresholds, before its smoothing) and of the reference image (before its smoothing and its
    once-only resample) on the GPU: cosmic-ray hits and hot pixels, which a global `small_fov_value_max` either misses or
    cuts together with bright real structure (include/coreg_hip.h: coreg_despike_small states the rule).  True (the
    defaults), a number of sigmas, or a dict of radius, nsigma, floor, min_neighbours, sign, replace, n_iter
    (utils/despiking.py: `despike_params`).  `self.last_despiked` = {"small": [...], "large": [...]} holds the pixels
    flagged per pass (those of the reference image cover the rectangle that was uploaded).  None changes nothing.
There is no CPU fallback: without the HIP library / a GPU the sweep raises.
"""
from __future__ import annotations

import copy
import os
import warnings

import numpy as np

from .. import _lib, parallel
from ..utils import diffrot, fits_io, header as hdrutil, wcs_tan
from ..utils.despiking import despike_params, despike_tag
from ..utils.smoothing import smoothing_tables
from .alignment_results import AlignmentResults


_METHODS = {"correlation": _lib.METHOD_CORRELATION,
            # alignment.py:544-547: no NaN mask, NaN unless every grid pixel overlaps
            "residus": _lib.METHOD_RESIDUS,
            "residus_masked": _lib.METHOD_RESIDUS_MASKED}


# A method of `align_using_carrington` only, recognised beside `_METHODS` (the helioprojective and plate-carree sweeps
# correct their noise-decided samples as slabs of Pearson sums: no histogram there, `library_method` has none)
MUTUAL_INFORMATION = "mutual_information"
DEFAULT_BINS, MAX_BINS = 16, 32


def library_method(name):
    """The library's method code of an `align_using_*` method name (alignment.py:549: anything else is not implemented)."""
    if name not in _METHODS:
        raise NotImplementedError
    return _METHODS[name]


def min_overlap_floor(min_overlap, counts=None):
    """The smallest sample count `min_overlap` admits: an integer >= 1 is that count, a float in (0, 1) a fraction of the
    largest finite entry of `counts` (NaN without one: nothing is admitted); anything else raises ValueError."""
    if isinstance(min_overlap, (int, np.integer)) and not isinstance(min_overlap, (bool, np.bool_)):
        if min_overlap < 1:
            raise ValueError("min_overlap as a count must be >= 1")
        return float(min_overlap)
    if isinstance(min_overlap, (float, np.floating)) and 0.0 < min_overlap < 1.0:
        finite = np.zeros(0) if counts is None else counts[np.isfinite(counts)]
        return float(min_overlap) * float(finite.max()) if finite.size else np.nan
    raise ValueError("min_overlap must be None, an integer >= 1 or a float in (0, 1)")


def parse_bins(method, bins):
    """The `bins` argument of `align_using_carrington`, checked without any image: None for every method but
    "mutual_information" (`bins` with another method raises ValueError); else an integer 2 <= B <= 32 (None: 16), or the
    pair (edges_small, edges_large) as `pxlshift.alignment_pixels.check_edges` returns them.  ValueError otherwise."""
    from ..pxlshift.alignment_pixels import check_edges
    if method != MUTUAL_INFORMATION:
        if bins is not None:
            raise ValueError("bins belongs to method='mutual_information'")
        return None
    if bins is None:
        return DEFAULT_BINS
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_)):
        if not 2 <= bins <= MAX_BINS:
            raise ValueError(f"bins as a number must lie in [2, {MAX_BINS}]")
        return int(bins)
    if isinstance(bins, (bool, np.bool_, float, np.floating, str)):
        raise ValueError("bins must be an integer or a pair (edges_small, edges_large)")
    try:
        es, el = bins
    except (TypeError, ValueError):
        raise ValueError("bins must be an integer or a pair (edges_small, edges_large)") from None
    return check_edges(es, "edges_small"), check_edges(el, "edges_large")


def default_edges(small_pixels, value_min, value_max, reference_on_grid, n_bins):
    """(edges_small, edges_large) of `n_bins` quantile bins (`pxlshift.alignment_pixels.quantile_edges`): of the image to
    align after the thresholds `small_fov_value_min` / `small_fov_value_max` (alignment.py:876-887), and of the prepared
    reference on the target grid.  Plain numpy on the images, thresholds and grid: no lag, slice or rank enters."""
    from ..pxlshift.alignment_pixels import quantile_edges
    small = np.array(small_pixels, dtype=np.float64)
    hdrutil.set_threshold_minmax_to_nan(small, value_min, value_max)
    return quantile_edges(small, int(n_bins)), quantile_edges(reference_on_grid, int(n_bins))


def apply_min_overlap(corr, counts, min_overlap):
    """The map with every lag-point of fewer than `min_overlap` samples set to NaN (pandas' `min_periods`).  `counts`:
    per-lag sample counts, shaped like `corr` (NaN: never evaluated -- such a lag-point goes too).  `min_overlap`: None
    (the map as it is) or as `min_overlap_floor` takes it.  ValueError when no finite entry is left."""
    if min_overlap is None:
        return corr
    corr = np.asarray(corr, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    if counts.shape != corr.shape:
        raise ValueError("min_overlap: the sample counts do not have the shape of the map")
    floor = min_overlap_floor(min_overlap, counts)
    with np.errstate(invalid="ignore"):
        keep = counts >= floor
    out = np.where(keep, corr, np.nan)
    if not np.isfinite(out).any():
        raise ValueError(f"min_overlap={min_overlap!r} leaves no lag-point of the sweep")
    return out


class Alignment:

    def __init__(self, large_fov_known_pointing, small_fov_to_correct, lag_crval1, lag_crval2, lag_cdelt1, lag_cdelt2,
                 lag_crota, lag_solar_r=None, small_fov_value_min=None, parallelism=False, display_progress_bar=False,
                 small_fov_value_max=None, counts_cpu_max=40, large_fov_window=-1, small_fov_window=-1,
                 path_save_figure=None, reprojection_order=2, force_crota_0=False, unit_lag="arcsec",
                 cdelt_semantics="intended", device=None, differential_rotation="reference", min_overlap=None,
                 smooth_small=None, smooth_large=None, smooth_unit="pixel", despike_small=None, despike_large=None):
        self.large_fov_known_pointing = large_fov_known_pointing
        self.small_fov_to_correct = small_fov_to_correct
        self.lag_crval1 = lag_crval1
        self.lag_crval2 = lag_crval2
        self.lag_cdelt1 = lag_cdelt1
        self.lag_cdelt2 = lag_cdelt2
        self.lag_crota = lag_crota
        self.lag_solar_r = lag_solar_r
        self.unit_lag = unit_lag
        self.unit_lag_input = copy.deepcopy(unit_lag)
        self.lonlims = None
        self.latlims = None
        self.shape = None
        self.reference_date = None
        self.parallelism = parallelism
        self.small_fov_window = small_fov_window
        self.large_fov_window = large_fov_window
        self.counts = counts_cpu_max
        self.small_fov_value_min = small_fov_value_min
        self.small_fov_value_max = small_fov_value_max
        self.path_save_figure = path_save_figure
        self.display_progress_bar = display_progress_bar
        self.force_crota_0 = force_crota_0
        self.order = reprojection_order
        self.method = None
        self.coordinate_frame = None
        self.data_large = self.data_small = self.hdr_large = self.hdr_small = None
        if cdelt_semantics not in ("intended", "reference"):
            raise ValueError("cdelt_semantics must be 'intended' or 'reference'")
        self.cdelt_semantics = cdelt_semantics
        if differential_rotation not in ("intended", "reference"):
            raise ValueError("differential_rotation must be 'intended' or 'reference'")
        self.differential_rotation = differential_rotation
        self.device = device
        # plain image HDUs of local files go to the GPU as the file stores them (COREG_RAW_FITS=0: decode on the host)
        self.raw_fits_upload = os.environ.get("COREG_RAW_FITS", "1") != "0"
        self.last_stats = None
        if min_overlap is not None:
            min_overlap_floor(min_overlap)  # (its checks, before anything is loaded)
        self.min_overlap = min_overlap  # lag-points with fewer samples become NaN (apply_min_overlap); None: no floor
        if smooth_unit not in ("pixel", "arcsec"):
            raise ValueError("smooth_unit must be 'pixel' or 'arcsec'")
        # (the form of both arguments, before anything is loaded; in arcsec the tables need the headers: `_smoothing`)
        for arg, what in ((smooth_small, "smooth_small"), (smooth_large, "smooth_large")):
            smoothing_tables(arg, what, (1.0, 1.0) if smooth_unit == "pixel" else (0.0, 0.0))
        self.smooth_small, self.smooth_large, self.smooth_unit = smooth_small, smooth_large, smooth_unit
        self._smooth_large_tables = None  # (wy, wx) of the sweep being run, None: none
        # (their checks, before anything is loaded) the rule of each image as a dict, None: none
        self.despike_small = despike_params(despike_small, "despike_small")
        self.despike_large = despike_params(despike_large, "despike_large")
        self.last_despiked = None       # {"small": [...], "large": [...]}: pixels flagged per pass in the last sweep
        self.last_counts = None         # per-lag sample counts of the last sweep, shaped like its map
        self.last_bins = None           # (edges_small, edges_large) of the last "mutual_information" sweep
        self._bins = None               # `bins` of the sweep being run, as parse_bins leaves it
        self.last_sharding = None       # how the last sweep was spread over the GPUs (parallel.lag_sharding)
        # set by the jitter-correction session (jitter_correction/jitter_correction.py):
        self.shard_lags = True          # False: every rank runs whole sweeps (images, not lags, are spread over GPUs)
        self._preloaded_small = None    # (data, header) already decoded by the session's prefetch thread
        self._handle_slot = 0           # which of the device's library contexts this sweep runs in
        # alignment.py:137-140
        for name in ("lag_crval1", "lag_crval2", "lag_crota", "lag_cdelt1", "lag_cdelt2"):
            if getattr(self, name) is None:
                setattr(self, name, np.array([0.0]))

    # ------------------------------------------------------------------------------------------------------------
    def _load(self):
        """Headers of both files and the pixels of the image to align.  The reference image's pixels are decoded only
        when `_large_pixels()` is called: a sweep whose prepared reference is still resident on the GPU never does."""
        self.data_large = None
        self.hdr_large = fits_io.Header(fits_io.read_header(self.large_fov_known_pointing, self.large_fov_window))
        if self._preloaded_small is not None:
            ds, hs = self._preloaded_small
        else:
            # a plain image HDU of a local file is not decoded on the host at all: its bytes are memory-mapped and go
            # to the GPU as the file stores them (fits_io.RawImage; byte swap, BSCALE / BZERO and the float conversion
            # of alignment.py:198 / :314 run there).  Anything else (in-memory pairs, compressed images, URLs with
            # astropy) is read and decoded as before.
            # A tile-compressed image (EUI level-1 / level-2 files) likewise: its COMPRESSED bytes go up and the GPU
            # decodes them (fits_io.CompressedImage; cfitsio's RICE_1 codec restated, csrc/ricecomp.hpp).
            ds, hs = (fits_io.load_for_upload if self.raw_fits_upload else fits_io.read_image)(
                self.small_fov_to_correct, self.small_fov_window)
        # float32 (BITPIX=-32) pixels stay float32: the float64 cast of alignment.py:198 / :314 is exact
        self.data_small = fits_io.native_pixels(ds)
        self.hdr_small = fits_io.Header(hs)
        hdrutil.check_and_create_pcij_matrix(self.hdr_small, self.force_crota_0)  # alignment.py:232 / :310
        hdrutil.check_and_create_pcij_matrix(self.hdr_large, self.force_crota_0)

    def _large_pixels(self):
        if self.data_large is None:
            dl = (fits_io.load_for_upload if self.raw_fits_upload else fits_io.read_image)(
                self.large_fov_known_pointing, self.large_fov_window)[0]
            # alignment.py:191 / :301 cast to float64; float32 pixels (BITPIX=-32) are kept as they are -- the cast is
            # exact and the library does it on the GPU, half the bytes cross PCIe; a memory-mapped data unit (RawImage)
            # goes up as stored, and only the rectangle the target grid can touch
            self.data_large = fits_io.native_pixels(dl)
        return self.data_large

    def _small_pixels_on_host(self):
        """The pixels of the image to align as loaded (a memory-mapped or tile-compressed data unit decoded on the host)."""
        d = self.data_small
        return d.decode() if isinstance(d, (fits_io.RawImage, fits_io.CompressedImage)) else np.asarray(d)

    def _reference_tag(self, frame, *what):
        """Identity of a prepared reference: (file identity of the reference image, preparation parameters), or None
        when the reference image is an in-memory array."""
        ident = fits_io.file_identity(self.large_fov_known_pointing, self.large_fov_window)
        if ident is None:
            return None

        def flat(v):
            return tuple(np.asarray(v, dtype=np.float64).ravel().tolist())
        return (ident, frame, bool(self.force_crota_0), int(self.order)) + tuple(flat(w) for w in what)

    def _carrington_tag(self, solar_r, rot_large):
        """Identity of the reference image on the Carrington grid: a resident one prepared for another rotation (another
        `reference_date`, another band) or with another smoothing or despiking is not this one.  (Without
        `despike_large` the tag is what it was before that keyword existed.)"""
        tag = self._reference_tag("carrington", self.lonlims, self.latlims, self.shape, solar_r, rot_large or (),
                                  *(self._smooth_large_tables or ()))
        return tag if tag is None or self.despike_large is None else tag + (despike_tag(self.despike_large),)

    def _smoothing(self, which):
        """(wy, wx) of `smooth_small` / `smooth_large` in pixels of that image's grid as its header stands, or None."""
        arg = self.smooth_small if which == "small" else self.smooth_large
        if arg is None:
            return None
        scale = (1.0, 1.0)
        if self.smooth_unit == "arcsec":
            hdr = self.hdr_small if which == "small" else self.hdr_large
            arcsec = hdrutil.unit_to_deg("arcsec")
            scale = (arcsec / abs(hdr["CDELT2"] * hdrutil.unit_to_deg(hdr["CUNIT2"])),
                     arcsec / abs(hdr["CDELT1"] * hdrutil.unit_to_deg(hdr["CUNIT1"])))
        return smoothing_tables(arg, "smooth_" + which, scale)

    def _rotations(self):
        """(rotation of the reference image, rotation of the image to align) of the Carrington frame, each
        (delta_t_days, c0, c1, c2) or None (utils/diffrot.py): None, None unless differential_rotation="intended"."""
        if self.differential_rotation != "intended" or self.coordinate_frame != "final_carrington":
            return None, None
        return (diffrot.rotation(self.hdr_large, self.hdr_large, self.reference_date),
                diffrot.rotation(self.hdr_small, self.hdr_large, self.reference_date))

    def _set_initial_header_values(self, ang2pipi=True):
        """alignment.py:799-842."""
        h = self.hdr_small
        self.crval1_ref, self.crval2_ref = h["CRVAL1"], h["CRVAL2"]
        if "CROTA" in h:
            self.crota_ref = h["CROTA"]
        elif "CROTA2" in h:
            self.crota_ref = h["CROTA2"]
        else:
            s = -np.sign(h["PC1_2"]) + (h["PC1_2"] == 0)
            self.crota_ref = np.rad2deg(np.arccos(h["PC1_1"])) * s
            h["CROTA"] = np.rad2deg(np.arccos(h["PC1_1"]))
        self.cdelt1_ref, self.cdelt2_ref = h["CDELT1"], h["CDELT2"]
        self.unit1, self.unit2 = str(h["CUNIT1"]).strip(), str(h["CUNIT2"]).strip()
        if self.unit_lag in self.unit1:
            pass
        else:
            warnings.warn("Units of headers in deg: Modyfying inputs units to deg.")
            for name, unit in (("lag_crval1", self.unit1), ("lag_crval2", self.unit2), ("lag_cdelt1", self.unit1),
                               ("lag_cdelt2", self.unit2)):
                v = np.asarray(getattr(self, name), dtype=np.float64)
                if ang2pipi:
                    v = hdrutil.ang2pipi(v, self.unit_lag)
                setattr(self, name, hdrutil.convert(v, self.unit_lag, unit))
            self.unit_lag = self.unit1
        if self.unit1 != self.unit2:
            raise ValueError("CUNIT1 and CUNIT2 must be equal")
        if self.lag_solar_r is None:
            self.lag_solar_r = np.array([1.004])

    # ------------------------------------------------------------------------------------------------------------
    def align_using_carrington(self, lonlims=None, latlims=None, size_deg_carrington=None, shape=None,
                               reference_date=None, method="correlation", method_carrington_reprojection="fa",
                               return_type="AlignmentResults", bins=None):
        """alignment.py:144-261.  `bins` (method "mutual_information" only, ValueError with any other): an integer
        2 <= B <= 32 (default 16) -- B quantile bins of the image to align after its thresholds and of the prepared
        reference on the grid for the first `lag_solar_r` (`default_edges`) -- or a pair (edges_small, edges_large) as
        `pxlshift.alignment_pixels.check_edges` takes them; the edges used are kept as `self.last_bins`.
        `reference_date` (default: DATE-AVG of the reference image) acts only with
        `differential_rotation="intended"`: each image is then rotated over (its DATE-OBS - reference_date), leap seconds
        inside that interval ignored, at the rate of the band the reference image's WAVELNTH selects (utils/diffrot.py)."""
        self._bins = parse_bins(method, bins)  # (refused before anything is loaded)
        self.method = method
        self.coordinate_frame = "final_carrington"
        if method_carrington_reprojection == "sunpy":
            raise NotImplementedError("method_carrington_reprojection='sunpy' delegates to sunpy.reproject_to in the "
                                      "reference (alignment.py:939-985) and is out of scope of the GPU path")
        if method_carrington_reprojection != "fa":
            raise ValueError("method_carrington_reprojection must be either 'fa' or 'sunpy")
        self._load()
        if reference_date is None:
            if "DATE-AVG" not in self.hdr_large:
                raise ValueError("Either provide a reference date manualy or the reference file header must have a "
                                 "DATE-AVG keyword.")
            self.reference_date = self.hdr_large["DATE-AVG"]
        else:
            # no numerical effect on the 'fa' path (quirk Q5) unless differential_rotation="intended"
            self.reference_date = reference_date
        if (lonlims is None) and (latlims is None) and (size_deg_carrington is not None):
            crln, crlt = self.hdr_small["CRLN_OBS"], self.hdr_small["CRLT_OBS"]
            self.lonlims = [crln - 0.5 * size_deg_carrington[0], crln + 0.5 * size_deg_carrington[0]]
            self.latlims = [crlt - 0.5 * size_deg_carrington[1], crlt + 0.5 * size_deg_carrington[1]]
            self.shape = [self.hdr_small["NAXIS1"], self.hdr_small["NAXIS2"]]
        elif (lonlims is not None) and (latlims is not None) and (shape is not None):
            self.lonlims, self.latlims, self.shape = lonlims, latlims, shape
        else:
            raise ValueError("either set lonlims as None, or not. no in between.")
        if self.shape[0] * self.shape[1] > 25000000:
            warnings.warn(f"shape parameter is {shape=}, which is very large.Computational time might significantly "
                          "increase")
        results = self._find_best_header_parameters()
        return self._wrap(results, return_type, restore_units=True)

    def align_using_helioprojective(self, method="correlation", return_type="AlignmentResults", fov_limits=None,
                                    remove_fov_limits=None):
        """alignment.py:263-342."""
        self.lonlims = self.latlims = self.shape = self.reference_date = None
        self.method = method
        self.coordinate_frame = "final_helioprojective"
        self._load()
        results = self._find_best_header_parameters(fov_limits=fov_limits, remove_fov_limits=remove_fov_limits)
        return self._wrap(results, return_type, restore_units=True)

    def align_using_initial_carrington(self, method="correlation", return_type="AlignmentResults"):
        """alignment.py:344-399: both inputs are already Carrington maps (CRLN-CAR / CRLT-CAR, plate carree).  The image
        reference map is resampled once on the pixel grid of the map to align (the sub-map of alignment.py:987-1016, in
        both the parallel and the serial branch), the map to align per lag on that same grid; no Carrington transform;
        both images are read as float32, lags are not wrapped (ang2pipi=False)."""
        self.lonlims = self.latlims = self.shape = self.reference_date = None
        self.method = method
        self.coordinate_frame = "initial_carrington"
        self._load()
        for hdr, what in ((self.hdr_small, "image to align"), (self.hdr_large, "reference image")):
            if not str(hdr.get("CTYPE1", "")).strip().upper().endswith("-CAR"):
                raise ValueError(f"align_using_initial_carrington: the {what} is not a CRLN-CAR / CRLT-CAR map")
        self.data_small = np.array(self.data_small, dtype=np.float32)  # alignment.py:384
        results = self._find_best_header_parameters(ang2pipi=False)
        if return_type == "corr":
            return results
        return AlignmentResults(corr=results, lag_crval1=self.lag_crval1, lag_crval2=self.lag_crval2,
                                lag_cdelt1=self.lag_cdelt1, lag_cdelt2=self.lag_cdelt2, lag_crota=self.lag_crota,
                                unit_lag=self.unit_lag, image_to_align_path=self.small_fov_to_correct,
                                image_to_align_window=self.small_fov_window,
                                reference_image_path=self.large_fov_known_pointing,
                                reference_image_window=self.large_fov_window, **self._results_keywords())

    def _results_keywords(self):
        """What AlignmentResults is told beyond the reference's arguments: the sample counts, and that the best entry of
        a `residus_masked` map is its minimum (`residus` keeps the reference's argmax)."""
        return {"n_samples": self.last_counts, "best": "min" if self.method == "residus_masked" else "max"}

    def _wrap(self, results, return_type, restore_units):
        if return_type == "corr":
            return results
        if return_type != "AlignmentResults":
            return results
        if restore_units:  # alignment.py:242-250 / :325-333
            for name in ("lag_crval1", "lag_crval2", "lag_cdelt1", "lag_cdelt2"):
                v = hdrutil.ang2pipi(getattr(self, name), self.unit_lag)
                setattr(self, name, hdrutil.convert(v, self.unit_lag, self.unit_lag_input))
            self.unit_lag = self.unit_lag_input
        return AlignmentResults(corr=results, lag_crval1=self.lag_crval1, lag_crval2=self.lag_crval2,
                                lag_cdelt1=self.lag_cdelt1, lag_cdelt2=self.lag_cdelt2, lag_crota=self.lag_crota,
                                unit_lag=self.unit_lag_input, image_to_align_path=self.small_fov_to_correct,
                                image_to_align_window=self.small_fov_window,
                                reference_image_path=self.large_fov_known_pointing,
                                reference_image_window=self.large_fov_window, **self._results_keywords())

    # ------------------------------------------------------------------------------------------------------------
    def _set_remove_fov_limits_to_nan(self, remove_fov_limits):
        """alignment.py:863-874: pixels of the small image inside the lon/lat box -> NaN.  Limits: astropy Quantities
        or plain numbers in the input lag unit."""
        lon, lat = wcs_tan.pixel_lonlat(self.hdr_small)
        lonl = wcs_tan._lims_deg(remove_fov_limits[0], self.unit_lag_input)
        latl = wcs_tan._lims_deg(remove_fov_limits[1], self.unit_lag_input)
        inside = (lon >= lonl[0]) & (lon <= lonl[1]) & (lat >= latl[0]) & (lat <= latl[1])
        self.data_small[inside] = np.nan

    def _select_fov_in_small_data(self, fov_limits, handle):
        """alignment.py:1082-1127: re-grid the small image on a regular lon/lat grid restricted to `fov_limits`
        (new header: PC = identity, CROTA = 0).  Literal restatement, including the reference's use of the ROW count
        for CRPIX1 / NAXIS1 (it mixes the two axes, harmless for square selections).  The resample runs on the GPU."""
        h = self.hdr_small
        lon, lat = wcs_tan.pixel_lonlat(h)
        lonl = wcs_tan._lims_deg(fov_limits[0], self.unit_lag_input)
        latl = wcs_tan._lims_deg(fov_limits[1], self.unit_lag_input)
        long, latg, dlon, dlat = wcs_tan.build_regular_grid(lon, lat, lonl, latl)
        if long.size == 0:
            raise ValueError("fov_limits select no pixel of the small image")
        mid = [long.shape[0] // 2, long.shape[1] // 2]
        hg = h.copy()
        u1, u2 = hdrutil.unit_to_deg(h["CUNIT1"]), hdrutil.unit_to_deg(h["CUNIT2"])
        hg["CRVAL1"] = float(long[mid[0], mid[1]]) / u1
        hg["CRVAL2"] = float(latg[mid[0], mid[1]]) / u2
        hg["CRPIX1"] = mid[0] + 1
        hg["CRPIX2"] = mid[1] + 1
        hg["CDELT1"] = float(dlon) / u1
        hg["CDELT2"] = float(dlat) / u2
        hg["PC1_1"], hg["PC2_2"], hg["PC1_2"], hg["PC2_1"] = 1.0, 1.0, 0.0, 0.0
        hg["CROTA"] = 0.0
        hg["CROTA2"] = 0.0
        hg["NAXIS1"] = long.shape[0]
        hg["NAXIS2"] = long.shape[1]
        hg.pop("ZNAXIS1", None)
        hg.pop("ZNAXIS2", None)
        handle.set_small(self.data_small)
        self.data_small = handle.resample_helioprojective(hg, h, order=self.order, dtype=np.float64)
        self.hdr_small = hg

    def _find_best_header_parameters(self, ang2pipi=True, fov_limits=None, remove_fov_limits=None):
        """`_sweep`; the long-lived handle it ran on keeps neither this object's reference smoothing nor its reference
        despiking, whatever happened."""
        self._sweep_handle = None
        try:
            return self._sweep(ang2pipi, fov_limits, remove_fov_limits)
        finally:
            if self._sweep_handle is not None and self._smooth_large_tables is not None:
                self._sweep_handle.set_reference_smoothing(None)
            if self._sweep_handle is not None and self.despike_large is not None:
                self._sweep_handle.set_reference_despike(None)
            self._sweep_handle = None

    def _sweep(self, ang2pipi=True, fov_limits=None, remove_fov_limits=None):
        """alignment.py:613-797 on the GPU.  Returns float64 [n_crval1, n_crval2, n_cdelt1, n_cdelt2, n_crota,
        n_solar_r]; lag-points the library could not evaluate are NaN, never 0 (quirk Q9)."""
        mi = self.method == MUTUAL_INFORMATION
        if mi and self.coordinate_frame != "final_carrington":
            raise NotImplementedError("method='mutual_information' is a score of align_using_carrington only: the border and "
                                      "near-integer samples of the helioprojective and plate-carree sweeps are corrected as "
                                      "Pearson sums, which a histogram cannot take")
        method = _lib.METHOD_MUTUAL_INFORMATION if mi else library_method(self.method)
        device = self.device
        rank, world = parallel.world_info()
        if not self.shard_lags:
            rank, world = 0, 1
        if device is None:
            device = -1
            if parallel.world_info()[1] > 1:
                import torch
                device = torch.cuda.current_device()
        # A plain script (no torch.distributed) that asks for `parallelism=True` gets what the reference gives it: the whole
        # machine (alignment.py:692-744 fans out over counts_cpu_max processes).  Here: every visible GPU, driven from
        # this one process by the library itself (coreg_multi: a host thread + context per device, lag-plane blocks, one
        # RCCL all-gather).  An explicit `device=`, a jitter session spreading images over GPUs, one visible GPU or
        # COREG_SINGLE_DEVICE=1 keep the single-device context.
        use_all = (self.parallelism and world == 1 and self.device is None and self.shard_lags
                   and parallel.world_info()[1] == 1 and os.environ.get("COREG_SINGLE_DEVICE", "0") != "1"
                   and _lib.device_count() > 1 and not mi)  # (the histograms are the single-device handle's)
        if use_all:
            h = _lib.shared_multi_handle()
        else:
            h = _lib.shared_handle(device, self._handle_slot)  # long-lived: buffers are re-used by the next Alignment
        # with several ranks over RCCL each image crosses PCIe once in all -- 1/N per rank -- and is assembled on every
        # GPU by an all-gather over xGMI (parallel.replicate_image); one rank / gloo: the whole image from this host
        spread = world > 1

        def upload_small(data):
            if spread and isinstance(data, (fits_io.RawImage, fits_io.CompressedImage)):
                data = fits_io.native_pixels(data.decode())  # row shares + all-gather work on decoded pixels
            t = parallel.replicate_image(data) if spread and np.asarray(data).dtype in (np.float32, np.float64) else None
            if t is None:
                h.set_small(data)
            else:
                import torch
                torch.cuda.current_stream().synchronize()  # the all-gather ran on torch's stream, not the handle's
                h.set_small_from_device(t.data_ptr(), t.shape, np.float32 if t.element_size() == 4 else np.float64)
                h.synchronize()  # `t` may go once the copy has run

        # the handle is long-lived and keeps its rotations: set on every call, None included
        rot_large, rot_small = self._rotations()
        if self.coordinate_frame == "final_carrington":
            h.set_rotation("reference", rot_large)
            h.set_rotation("small", rot_small)
        # ... and its reference smoothing
        self._smooth_large_tables = self._smoothing("large")
        self._sweep_handle = h
        h.set_reference_smoothing(self._smooth_large_tables)
        # ... and its reference despiking (set only where the keyword is: None runs no new code)
        if self.despike_large is not None:
            h.set_reference_despike(self.despike_large)
        self.last_despiked = {"small": [], "large": []}
        # alignment.py:844-861: thresholds, then the box to remove, then the sub-FOV re-grid
        on_device = (remove_fov_limits is None) and (fov_limits is None)
        n_finite = None
        if on_device:
            # thresholds applied to the resident copy (self.data_small is left as loaded).  The upload runs on the handle's
            # upload stream; the threshold pass -- the first reader of the pixels -- is issued after the reference
            # preparation (`finite_pixels`, below), which therefore does not wait for the image's DMA.
            # COREG_ASYNC_UPLOAD=1 also hands the staging copies to the library's upload thread (option "async_upload";
            # measured +-0.03 ms on the headline call -- the DMA already overlaps the preparation -- hence off by default).
            # self.data_small is not modified until the sweep has returned.
            # (only when a reference preparation follows -- nothing to overlap with when the prepared reference is still
            # resident, and the hand-over to the thread then costs more than it saves: profiles/r05_api_timing*.json)
            will_prepare = True
            if self.coordinate_frame == "final_carrington":
                sr0 = 1.004 if self.lag_solar_r is None else float(np.atleast_1d(self.lag_solar_r)[0])
                tag0 = self._carrington_tag(sr0, rot_large)
                will_prepare = tag0 is None or tag0 != getattr(h, "reference_tag", None)
            use_async = (will_prepare and not use_all and not spread
                         and os.environ.get("COREG_ASYNC_UPLOAD", "0") == "1")
            if use_async:
                h.set_option("async_upload", 1)
            try:
                upload_small(self.data_small)
            finally:
                if use_async:
                    h.set_option("async_upload", 0)
        else:
            self.data_small = np.array(self.data_small, dtype=np.float64)
            hdrutil.set_threshold_minmax_to_nan(self.data_small, self.small_fov_value_min, self.small_fov_value_max)
            if remove_fov_limits is not None:
                self._set_remove_fov_limits_to_nan(remove_fov_limits)
            if fov_limits is not None:
                self._select_fov_in_small_data(fov_limits, h)
            n_finite = int(np.isfinite(self.data_small).sum())
            upload_small(self.data_small)
        smooth_small = self._smoothing("small")  # (of the header the image now has: a sub-FOV re-grid changes CDELT)
        self._set_initial_header_values(ang2pipi)

        def finite_pixels():
            """alignment.py:654-656, after the first reference preparation (the check itself reads the uploaded pixels).
            The despiking of the image to align follows its thresholds and its smoothing follows both: a masked pixel
            is no neighbour and cannot bleed, a spike is cut before it can be spread."""
            nonlocal n_finite, smooth_small, despike_small
            if n_finite is None:
                n_finite = h.threshold_small(self.small_fov_value_min, self.small_fov_value_max)
            if n_finite == 0:
                raise ValueError("minimum or maximum value have set all small FOV to nan")
            if despike_small is not None:
                self.last_despiked["small"] = h.despike_small(despike_small)
                smoothed_small[0], despike_small = True, None
            if smooth_small is not None:
                h.smooth_small(smooth_small)
                smoothed_small[0], smooth_small = True, None

        smoothed_small = [False]  # the resident image is no longer the thresholded file's: despiked, smoothed or both
        despike_small = self.despike_small

        if n_finite is not None:
            finite_pixels()
        if self.unit_lag != self.hdr_small["CUNIT1"]:
            raise ValueError("lag.unit and cUNIT are not the same")  # alignment.py:406

        lags = _lib.LagSet(self.lag_crval1, self.lag_crval2, self.lag_cdelt1, self.lag_cdelt2, self.lag_crota)
        sem = _lib.CDELT_INTENDED if self.cdelt_semantics == "intended" else _lib.CDELT_REFERENCE
        solar_rs = np.atleast_1d(np.asarray(self.lag_solar_r, dtype=np.float64))
        # Spreading the lag set over the GPUs (parallel.lag_sharding): blocks of the (CRVAL1, CRVAL2) plane + one
        # all-gather -- the partition bench.py measures; contiguous slices of the raveled index (the reference's literal
        # np.array_split, alignment.py:677-687) when the plane is smaller than the number of GPUs; shares of the GRID +
        # one all-reduce of the six sums per lag when there are few lag-points per GPU.
        # (the helioprojective sweep runs ONE launch whatever the lag set; the others one per (cdelt, crota) combination)
        per_combo = self.coordinate_frame != "final_helioprojective"
        mode = parallel.lag_sharding(lags.shape, world, per_combo)
        if mi and mode == "points":
            mode = "slices"  # (six sums can be all-reduced; per-rank histograms are not part of the library)
        self.last_sharding = mode
        my_lags, lo, hi = lags, 0, lags.size
        combos = None  # (c_lo, c_hi): this rank's run of (cdelt1, cdelt2, crota) combinations, None = all of them
        if mode in ("blocks", "combos"):
            lo1, hi1, lo2, hi2, c_lo, c_hi = parallel.grid_share(lags.shape, world, rank, per_combo)
            a = lags.arrays
            my_lags = _lib.LagSet(a[0][lo1:hi1], a[1][lo2:hi2], a[2], a[3], a[4])
            inner = lags.shape[2] * lags.shape[3] * lags.shape[4]
            if (c_lo, c_hi) != (0, inner):
                combos = (c_lo, c_hi)
            hi = my_lags.shape[0] * my_lags.shape[1] * (c_hi - c_lo)
        elif mode == "slices":
            lo, hi, _ = parallel.shard_bounds(lags.size, world, rank)

        def select_combos():
            if combos is not None:  # one-shot options, consumed by the sweep call that follows
                h.set_option("combo_begin", combos[0])
                h.set_option("combo_end", combos[1])

        def prepare(kind, *args):
            """Once-only reference preparation.  The library uploads only the rectangle of the reference image the target
            grid can touch (usually a few hundred KB), so every rank simply sends its own crop: nothing to replicate."""
            getattr(h, "prepare_reference_" + kind)(self._large_pixels(), *args)

        out = np.full(lags.shape + (len(solar_rs),), np.nan)
        counts = np.full(out.shape, np.nan)
        on_grid_despiked = False  # the reference was despiked in the pixel-lag sweep's image slot, its counts are taken
        for kk, solar_r in enumerate(solar_rs):
            if self.coordinate_frame == "final_carrington":
                grid = _lib.Grid(self.lonlims, self.latlims, self.shape, numpy_lat_trig=True)
                tag = self._carrington_tag(solar_r, rot_large)
                if tag is None or tag != h.reference_tag:
                    prepare("carrington", self.hdr_large, grid, solar_r, self.order)
                    h.reference_tag = tag

                def run(g=grid, sr=solar_r):
                    select_combos()
                    return h.sweep_carrington(self.hdr_small, g, sr, my_lags, order=self.order, method=method,
                                              cdelt_semantics=sem, lag_begin=lo, lag_end=hi)
            elif self.coordinate_frame == "initial_carrington":
                # BOTH branches of the reference name this frame in their sub-map condition (alignment.py:649-651 parallel,
                # :765-767 serial): the reference map is resampled once on the grid of the map to align, float32, and
                # every lag re-samples the map to align on its own grid (round 5: found by the reference-run fixtures;
                # rounds 1-4 correlated on the reference map's full grid)
                # the reference casts the reference map to float32 BEFORE the sub-map interpolation in this frame
                # (alignment.py:371-372); exact and free for BITPIX=-32 pixels, a rounding for a float64 map
                big = self._large_pixels()
                if getattr(big, "dtype", None) != np.float32:  # (also a memory-mapped data unit that is not BITPIX=-32)
                    big = np.asarray(big).astype(np.float32)
                h.prepare_reference_helioprojective(big, self.hdr_large, self.hdr_small, self.order)

                def run():
                    select_combos()
                    return h.sweep_helioprojective(self.hdr_small, self.hdr_small, my_lags, order=self.order,
                                                   method=method, cdelt_semantics=sem, lag_begin=lo, lag_end=hi)
            else:
                if self.parallelism:
                    prepare("helioprojective", self.hdr_large, self.hdr_small, self.order)
                    target = self.hdr_small
                else:
                    big = np.asarray(self._large_pixels(), dtype=np.float64)  # quirk Q1: float64
                    if self._smooth_large_tables is not None or self.despike_large is not None:
                        # no resample here, so no preparation to despike or smooth in: the pixel-lag sweep's image slot serves
                        h.pixels_set_large(big)
                        if self.despike_large is not None:
                            self.last_despiked["large"] = h.pixels_despike_large(self.despike_large)
                        if self._smooth_large_tables is not None:
                            h.pixels_smooth_large(self._smooth_large_tables)
                        big = h.pixels_get_image("large", big.shape)
                        on_grid_despiked = True
                    h.set_reference_on_grid(big)
                    target = self.hdr_large

                def run(t=target):
                    select_combos()
                    return h.sweep_helioprojective(t, self.hdr_small, my_lags, order=self.order, method=method,
                                                   cdelt_semantics=sem, lag_begin=lo, lag_end=hi)
            finite_pixels()
            if mi and kk == 0:
                edges = self._bins
                if isinstance(edges, int):
                    ref_on_grid = h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64)
                    if smoothed_small[0]:  # the smoothed image, read back (its thresholds are in it)
                        edges = default_edges(h.get_small(tuple(np.shape(self.data_small))), None, None, ref_on_grid, edges)
                    else:
                        edges = default_edges(self._small_pixels_on_host(), self.small_fov_value_min,
                                              self.small_fov_value_max, ref_on_grid, edges)
                h.sweep_set_bins(*edges)
                self.last_bins = edges
            # (the sample counts of this rank's share are gathered the way its coefficients are)
            if mode == "points":
                part = parallel.point_sharded_sweep(h, run, lags.size)
                n_part = h.last_counts()  # (every rank finalises the reduced sums)
            elif mode in ("blocks", "combos"):
                part = parallel.allgather_lag_blocks(run(), lags.shape, per_combo_launch=per_combo)
                n_part = parallel.allgather_lag_blocks(h.last_counts(), lags.shape, per_combo_launch=per_combo)
            elif mode == "slices":
                part = parallel.allgather_lag_slices(run(), lags.size).cpu().numpy()
                n_part = parallel.allgather_lag_slices(h.last_counts(), lags.size).cpu().numpy()
            else:
                part = run()
                n_part = h.last_counts()
            out[..., kk] = np.asarray(part).reshape(lags.shape)
            counts[..., kk] = np.asarray(n_part).reshape(lags.shape)
        self.last_counts = counts
        if self.despike_large is not None and not on_grid_despiked:
            # (of the last preparation: the one this sweep ran, or the one that left the resident reference it re-used)
            self.last_despiked["large"] = h.last_reference_despike()[:self.despike_large["n_iter"]]
        out = apply_min_overlap(out, counts, self.min_overlap)
        self.last_stats = h.last_stats()
        if hasattr(h, "drop_small_keepalive"):
            h.drop_small_keepalive()  # (every sweep has returned: the upload thread is done with the pixels)
        if use_all:
            self.last_sharding = h.last_mode
        elif self.coordinate_frame != "final_carrington" and hasattr(h, "last_tap_fix"):
            #  samples whose coordinate comes back within 1e-8 px of an integer (odd spline orders) or of a
            # bound of the image (even orders) are re-evaluated with wcslib's own arithmetic; a list beyond "tap_cap"
            # entries is not applied -- say so
            if h.last_tap_fix()["overflow"]:
                warnings.warn("more noise-decided samples than the library's 'tap_cap': isolated lag-points of this "
                              "sweep may differ from the reference by up to 1e-5 (raise it with set_option('tap_cap', n))")
        return out
