"""
`AlignmentSpice` -- drop-in for euispice_coreg.hdrshift.AlignmentSpice (hdrshift/alignment_spice.py:13-355): aligns a
SPICE L2 raster (4-D cube [time, wavelength, y, x]) or an L3 coefficient map with an imager / synthetic raster.  The
data preparation either side of the sweep (cube collapse over a wavelength interval, slit-edge masking, 4-D -> 2-D
header) is restated here without astropy; the sweep itself is the GPU path of `Alignment`.

Differences from the reference, all deliberate:
  * `sub_fov_window` compares longitudes wrapped to (-180, 180] deg (the reference compares wcslib's raw output, whose
    branch follows the sign of CRVAL1, against the user's limits);
  * the sunpy branch (alignment_spice.py:300-303) is not implemented;
  * inputs may be FITS paths or (data, header) pairs (then pass `level=`).

Beyond the reference: `despike_planes=` (level 2 only; `utils.despiking.despike_planes_params`: True, a number of sigmas or
a dict).  A cosmic-ray hit lands in one wavelength plane, and in the sum over the planes its contrast is diluted by the
noise of all the others, where `despike_small=` -- which sees the summed image -- cannot find it.  With the keyword every
selected plane is despiked on its own on the GPU, between the slit edges only (rows outside are never neighbours), and the
planes are summed there (include/coreg_hip.h: coreg_despike_sum_planes_be); everything after the sum is unchanged.
`last_despiked_planes` holds the flag events per pass, `despiked_plane_events` their int32 map on the 2-D image's grid
(zero in rows that were not processed).  Without the keyword the host sum runs, bit for bit as before.
"""
from __future__ import annotations

import datetime as _dt

import numpy as np

from .. import _lib
from ..utils import fits_io, header as hdrutil, spice_header, wcs_tan
from ..utils.despiking import despike_planes_params
from .alignment import Alignment, apply_min_overlap, library_method, parse_bins


def _angstrom(v):
    return float(v.to("angstrom").value) if hasattr(v, "to") else float(v)


def despiked_plane_sum(planes, sel, rule, rows, device=None, slot=0):
    """The planes `sel` of `planes` [n_planes, ny, nx] despiked one by one by `rule` over the rows [rows[0], rows[1]) and
    summed over the planes on the GPU (`CoregHandle.despike_sum_planes`): (image float64 [ny, nx], NaN outside the rows;
    flag events per pixel int32 [ny, nx], zero outside the rows; flag events per pass)."""
    ny, nx = planes.shape[1:]
    r0, r1 = rows
    image = np.full((ny, nx), np.nan, dtype=np.float64)
    events = np.zeros((ny, nx), dtype=np.int32)
    counts = [0] * int(rule["n_iter"])
    if r1 > r0:
        h = _lib.shared_handle(-1 if device is None else device, slot)
        image[r0:r1], events[r0:r1], counts = h.despike_sum_planes(planes, sel, rule, rows=(r0, r1))
    return image, events, counts


class AlignmentSpice(Alignment):

    def __init__(self, large_fov_known_pointing, small_fov_to_correct, lag_crval1=None, lag_crval2=None,
                 lag_cdelt1=None, lag_cdelt2=None, lag_crota=None, lag_solar_r=None, large_fov_window=-1,
                 small_fov_window=-1, parallelism=False, counts_cpu_max=40, display_progress_bar=False,
                 path_save_figure=None, wavelength_interval_to_sum="all", sub_fov_window="all", level=None,
                 cdelt_semantics="intended", device=None, differential_rotation="reference", min_overlap=None,
                 smooth_small=None, smooth_large=None, smooth_unit="pixel", despike_small=None, despike_large=None,
                 despike_planes=None):
        super().__init__(large_fov_known_pointing=large_fov_known_pointing, small_fov_to_correct=small_fov_to_correct,
                         lag_crval1=lag_crval1, lag_crval2=lag_crval2, lag_cdelt1=lag_cdelt1, lag_cdelt2=lag_cdelt2,
                         lag_crota=lag_crota, display_progress_bar=display_progress_bar, lag_solar_r=lag_solar_r,
                         parallelism=parallelism, counts_cpu_max=counts_cpu_max, large_fov_window=large_fov_window,
                         small_fov_window=small_fov_window, path_save_figure=path_save_figure,
                         cdelt_semantics=cdelt_semantics, device=device, differential_rotation=differential_rotation,
                         min_overlap=min_overlap, smooth_small=smooth_small, smooth_large=smooth_large,
                         smooth_unit=smooth_unit, despike_small=despike_small, despike_large=despike_large)
        self.sub_fov_window = sub_fov_window
        self.extend_pixel_size = None
        self.cut_from_center = None
        self.wavelength_interval_to_sum = wavelength_interval_to_sum
        self.level = level
        self.despike_planes = despike_planes_params(despike_planes, "despike_planes")
        self.last_despiked_planes = None   # flag events per pass of the last level-2 preparation with `despike_planes`
        self.despiked_plane_events = None  # ... per pixel of the 2-D image, int32

    # ------------------------------------------------------------------------------------------------------------
    def _level(self):
        """alignment_spice.py:94-98: from the file name, unless given."""
        if self.level is not None:
            return self.level
        name = self.small_fov_to_correct if isinstance(self.small_fov_to_correct, str) else ""
        if "L2" in name:
            return 2
        if "L3" in name:
            return 3
        return None

    def align_using_helioprojective(self, method="correlation", extend_pixel_size=False, cut_from_center=None,
                                    return_type="AlignmentResults", coefficient_l3=None):
        """alignment_spice.py:66-120."""
        self.lonlims = self.latlims = self.shape = self.reference_date = None
        self.method = method
        self.coordinate_frame = "final_helioprojective"
        self.extend_pixel_size = extend_pixel_size
        self.cut_from_center = cut_from_center
        self._extract_imager_data_header()
        self._extract_spice_data_header(level=self._level(), coeff=coefficient_l3)
        results = self._find_best_header_parameters()
        return self._wrap(results, return_type, restore_units=True)

    def align_using_carrington(self, lonlims, latlims, size_deg_carrington=None, shape=None, reference_date=None,
                               method="correlation", return_type="AlignmentResults", coefficient_l3=None, bins=None):
        """alignment_spice.py:122-180.  `method="mutual_information"` and its `bins`: as on
        `Alignment.align_using_carrington` -- the score for a SPICE line against an imager passband of another temperature.
        (The reference reads hdr_small before it is loaded when only
        `size_deg_carrington` is given; here the SPICE header is loaded first.)"""
        self._bins = parse_bins(method, bins)  # (refused before anything is loaded)
        self.reference_date = reference_date
        self.extend_pixel_size = False
        self.method = method
        self.coordinate_frame = "final_carrington"
        self._extract_imager_data_header()
        self._extract_spice_data_header(level=self._level(), coeff=coefficient_l3)
        if (lonlims is None) and (latlims is None) and (size_deg_carrington is not None):
            crln, crlt = self.hdr_small["CRLN_OBS"], self.hdr_small["CRLT_OBS"]
            self.lonlims = [crln - 0.5 * size_deg_carrington[0], crln + 0.5 * size_deg_carrington[0]]
            self.latlims = [crlt - 0.5 * size_deg_carrington[1], crlt + 0.5 * size_deg_carrington[1]]
            self.shape = [self.hdr_small["NAXIS1"], self.hdr_small["NAXIS2"]]
        elif (lonlims is not None) and (latlims is not None) and (shape is not None):
            self.lonlims, self.latlims, self.shape = lonlims, latlims, shape
        else:
            raise ValueError("either set lonlims as None, or not. no in between.")
        h = self.hdr_small  # alignment_spice.py:159-168: the Carrington transform works in arcsec
        for k in ("CRVAL1", "CRVAL2"):
            h[k] = float(hdrutil.convert(hdrutil.ang2pipi(h[k], h["CUNIT" + k[-1]]), h["CUNIT" + k[-1]], "arcsec"))
        for k in ("CDELT1", "CDELT2"):
            h[k] = float(hdrutil.convert(h[k], h["CUNIT" + k[-1]], "arcsec"))
        h["CUNIT1"] = h["CUNIT2"] = "arcsec"
        results = self._find_best_header_parameters()
        return self._wrap(results, return_type, restore_units=False)

    # ------------------------------------------------------------------------------------------------------------
    def _extract_imager_data_header(self):
        """alignment_spice.py:182-187."""
        # (the pixels are read when the reference is prepared -- `Alignment._large_pixels`: as stored, cropped to what the
        # target grid can touch, decoded on the GPU; not at all when the prepared reference is still resident)
        self.data_large = None
        self.hdr_large = fits_io.Header(fits_io.read_header(self.large_fov_known_pointing, self.large_fov_window))
        hdrutil.check_and_create_pcij_matrix(self.hdr_large, self.force_crota_0, warn=False)

    def _extract_spice_data_header(self, level, coeff=None):
        """alignment_spice.py:189-221."""
        # a big-endian view of the memory-mapped window: only the wavelength planes the sum needs are ever touched
        cube, hdr = fits_io.open_cube(self.small_fov_to_correct, self.small_fov_window)
        hdr = fits_io.Header(hdr)
        dt = hdr["PC4_1"]
        if level == 2:
            self._prepare_spice_from_l2(cube, hdr)
        elif level == 3:
            if self.despike_planes is not None:
                raise ValueError("despike_planes: a level-3 map has no wavelength planes to despike (level 2 only)")
            self._prepare_spice_from_l3(cube, hdr, coeff)
        else:
            raise ValueError("level must be 2 or 3")
        for k in ("SOLAR_B0", "RSUN_REF", "DSUN_OBS", "CROTA"):
            self.hdr_small[k] = hdr[k]
        for k in ("CRLN_OBS", "CRLT_OBS"):  # needed by the Carrington transform (rectify.py:387-415)
            if k in hdr and k not in self.hdr_small:
                self.hdr_small[k] = hdr[k]
        if self.extend_pixel_size:
            self._correct_solar_rotation(dt)
        hdrutil.check_and_create_pcij_matrix(self.hdr_small, self.force_crota_0, warn=False)

    def _correct_solar_rotation(self, dt):
        """alignment_spice.py:223-248: shrink CDELT1 by the apparent solar rotation during one raster step."""
        h = self.hdr_small
        B0 = np.deg2rad(h["SOLAR_B0"])
        band = self.hdr_large["WAVELNTH"]
        omega_car = np.deg2rad(360 / 25.38 / 86400)
        if band == 174:
            band = 171
        omega = omega_car + spice_header.diff_rot(B0, f"EIT {band}")
        Rsun, Dsun = h["RSUN_REF"], h["DSUN_OBS"]
        phi_rot = np.rad2deg(1.004 * omega * Rsun / (Dsun - 1.004 * Rsun)) * 3600  # arcsec / s
        alpha = np.deg2rad(h["CRVAL1"] * hdrutil.unit_to_deg(h["CUNIT1"]))
        phi = np.arcsin(((Dsun - 1.004 * Rsun) / (1.004 * Rsun)) * np.sin(alpha))
        dtx_old = float(hdrutil.convert(h["CDELT1"], h["CUNIT1"], "arcsec"))
        dtx_new = dtx_old - dt * phi_rot * np.cos(phi)
        h["CDELT1"] = float(hdrutil.convert(dtx_new, "arcsec", h["CUNIT1"]))

    def _prepare_spice_from_l2(self, cube, hdr):
        """alignment_spice.py:250-323."""
        cube = np.asarray(cube)
        if cube.ndim != 4:
            raise ValueError("a SPICE L2 window is a 4-D cube [time, wavelength, y, x]")
        ymin, ymax = spice_header.vertical_edges_limits(hdr)
        self.hdr_small = spice_header.celestial_header(hdr)
        # np.nansum(float64(cube)[0, sel], axis=0) of the reference, plane by plane in the same order (a reduction over
        # the outer axis is a sequential accumulation, so the sums are the same to the bit) without a float64 copy of the
        # whole cube; the rows outside [ymin, ymax) are NaN in the result either way
        if isinstance(self.wavelength_interval_to_sum, str) and self.wavelength_interval_to_sum == "all":
            sel = np.arange(cube.shape[1])
        elif isinstance(self.wavelength_interval_to_sum, (list, tuple)):
            wave = spice_header.wavelengths_angstrom(hdr)
            lo, hi = (_angstrom(v) for v in self.wavelength_interval_to_sum)
            sel = np.flatnonzero(np.logical_and(wave >= lo, wave <= hi))
        else:
            raise ValueError("wavelength_interval_to_sum must be a [wave_min * u.angstrom, wave_max * u.angstrom] "
                             "or 'all' str ")
        # big-endian float planes straight from the memory-mapped data unit: the library's threaded host routine (same
        # additions in the same order); anything else (native arrays handed over in memory, integer cubes): NumPy
        self.last_despiked_planes = self.despiked_plane_events = None
        if self.despike_planes is not None:
            # every selected plane despiked on its own between the slit edges, then the same sum, on the GPU; what follows
            # sets the rows outside [ymin, ymax) to NaN again
            r0, r1, _ = slice(ymin, ymax).indices(cube.shape[2])
            self.data_small, self.despiked_plane_events, self.last_despiked_planes = despiked_plane_sum(
                cube[0], sel, self.despike_planes, (r0, max(r0, r1)), self.device, self._handle_slot)
        else:
            self.data_small = _lib.nansum_planes_be(cube[0], sel)
        if self.data_small is None:
            self.data_small = np.zeros(cube.shape[2:], dtype=np.float64) if len(sel) == 0 else None
            for plane in cube[0][sel]:
                # NaN -> 0 on the plane in its own precision (native byte order), the float64 cast inside the addition:
                # same values, same order of additions as np.nansum(float64(cube)), in two light passes per plane
                if plane.dtype.kind == "f":
                    q = plane.astype(plane.dtype.newbyteorder("="))
                    np.copyto(q, 0, where=np.isnan(q))
                else:
                    q = plane
                if self.data_small is None:
                    self.data_small = q.astype(np.float64)
                else:
                    np.add(self.data_small, q, out=self.data_small)
        self.data_small[:ymin, :] = np.nan
        self.data_small[ymax:, :] = np.nan
        if self.cut_from_center is not None:
            xlen = self.cut_from_center
            xmid = self.data_small.shape[1] // 2
            self.data_small[:, :(xmid - xlen // 2 - 1)] = np.nan
            self.data_small[:, (xmid + xlen // 2):] = np.nan
        self.hdr_small["NAXIS1"] = self.data_small.shape[1]
        self.hdr_small["NAXIS2"] = self.data_small.shape[0]
        if isinstance(self.sub_fov_window, str) and self.sub_fov_window == "all":
            pass
        elif isinstance(self.sub_fov_window, (list, tuple)):
            lon, lat = wcs_tan.pixel_lonlat(self.hdr_small)
            lon = hdrutil.ang2pipi(lon)
            lonl = wcs_tan._lims_deg(self.sub_fov_window[0:2], "arcsec")
            latl = wcs_tan._lims_deg(self.sub_fov_window[2:4], "arcsec")
            sel = (lon >= lonl[0]) & (lon <= lonl[1]) & (lat >= latl[0]) & (lat <= latl[1])
            self.data_small[~sel] = np.nan
        else:
            raise ValueError("sub_fov_window must be a [lon_min * u.arcsec, lon_max * u.arcsec,"
                             " lat_min * u.arcsec, lat_max * u.arcsec] or 'all' str ")

    def _prepare_spice_from_l3(self, cube, hdr, coeff):
        """alignment_spice.py:340-355.  (NAXIS1/2 are set here; the reference leaves them out of the 2-D header.)"""
        self.data_small = np.array(np.asarray(cube)[coeff, ...], dtype=np.float64)  # (only the plane asked for)
        ymin, ymax = spice_header.vertical_edges_limits(hdr)
        self.data_small[:ymin, :] = np.nan
        self.data_small[ymax:, :] = np.nan
        self.hdr_small = spice_header.celestial_header(hdr)
        self.hdr_small["NAXIS1"] = self.data_small.shape[-1]
        self.hdr_small["NAXIS2"] = self.data_small.shape[-2]


class AlignementSpiceIterativeContextRaster(AlignmentSpice):
    """Drop-in for euispice_coreg.hdrshift.AlignementSpiceIterativeContextRaster (alignment_spice.py:357-469): the
    context image is composed anew for every candidate header -- each raster column an order-2 sample of the imager
    frame nearest in time to that slit, at the SHIFTED SPICE pointing (SPICEComposedMapBuilder.process_from_header) --
    and the SPICE image is resampled onto that grid and correlated with it (`_step`, :361-421).  The whole lag sweep is
    one library call (include/coreg_hip.h: coreg_sweep_context); every imager file is read once per call and the frames
    the raster uses stay resident on the GPU.

    Differences from the reference, all deliberate:
      * the reference cannot run as committed: its __init__ passes `use_tqdm`, `small_fov_value_min` /
        `small_fov_value_max` to an AlignmentSpice.__init__ that takes none of them, and align_using_helioprojective
        passes `index_amplitude=` to `_extract_spice_data_header(level, coeff)` (TypeError either way); its map builder
        returns os.path.join(None, ...) from process_from_header (TypeError after the map is made); its `_step`
        shifts the 4-D SPICE header, whose CUNIT is arcsec, with lags already converted to the flattened header's
        degrees, and _shift_header raises "lag.unit and cUNIT are not the same"; and the serial branch of its sweep
        driver never calls `_step` at all (alignment.py:765-797 calls `_step_no_shmm`).  Here every lag-point does what
        `_step` says, with the 4-D header's celestial cards taken in degrees;
      * `parallelism` is accepted and the sweep runs on one GPU (multi-GPU sharding of this sweep is not implemented);
      * level-3 input raises NotImplementedError (the reference's `_prepare_spice_from_l3` never sets the unflattened
        header its `_extract_imager_data_header` reads: AttributeError);
      * `cdelt_semantics` as on `Alignment` (default "intended"; "reference" reproduces _shift_header's CDELT handling).
    """

    def __init__(self, large_fov_list_paths, small_fov_to_correct, threshold_time, lag_crval1, lag_crval2, lag_cdelt1,
                 lag_cdelt2, lag_crota, small_fov_value_min=None, parallelism=False, small_fov_value_max=None,
                 counts_cpu_max=40, large_fov_window=-1, small_fov_window=-1, use_tqdm=False, path_save_figure=None,
                 cdelt_semantics="intended", device=None, min_overlap=None, despike_planes=None):
        super().__init__(large_fov_known_pointing="No_specific_path", small_fov_to_correct=small_fov_to_correct,
                         lag_crval1=lag_crval1, lag_crval2=lag_crval2, lag_cdelt1=lag_cdelt1, lag_cdelt2=lag_cdelt2,
                         lag_crota=lag_crota, lag_solar_r=None, parallelism=parallelism, counts_cpu_max=counts_cpu_max,
                         large_fov_window=large_fov_window, small_fov_window=small_fov_window,
                         display_progress_bar=use_tqdm, path_save_figure=path_save_figure,
                         cdelt_semantics=cdelt_semantics, device=device, min_overlap=min_overlap,
                         despike_planes=despike_planes)
        self.small_fov_value_min = small_fov_value_min
        self.small_fov_value_max = small_fov_value_max
        self.step_figure = False
        self.large_fov_list_paths = list(large_fov_list_paths)
        self.threshold_time = threshold_time
        self.header_spice_unflattened = None
        self.col_frame = None  # imager file (index into large_fov_list_paths) of every raster column, after a call

    # ------------------------------------------------------------------------------------------------------------
    def _prepare_spice_from_l2(self, cube, hdr):
        """alignment_spice.py:467-469: keep the 4-D header, then prepare as AlignmentSpice does."""
        self.header_spice_unflattened = fits_io.Header(hdr).copy()
        super()._prepare_spice_from_l2(cube, hdr)

    def _frame_of_columns(self, hdr4, headers):
        """map_builder.py:95-110: the imager frame closest in time to every raster column (the time axis of the 4-D
        header, averaged along the slit), ValueError when none is within `threshold_time`.  The lags move only the
        celestial cards, so the choice is the same for every lag-point."""
        from ..synras.map_builder import _seconds
        col_seconds, t_ref = spice_header.column_times(hdr4)
        dates = [spice_header.parse_date(h["DATE-AVG"]) for h in headers]
        threshold = _seconds(self.threshold_time)
        out = np.empty(len(col_seconds), dtype=np.int64)
        for ii, s in enumerate(col_seconds):
            utc = t_ref + _dt.timedelta(seconds=float(s))
            dt = np.array([abs((utc - d).total_seconds()) for d in dates], dtype=np.float64)
            if dt.min() > threshold:
                raise ValueError(f"dt={dt.min()} s: Could not find imager sufficiently close in time")
            out[ii] = int(dt.argmin())
        return out

    @staticmethod
    def _celestial_degrees(hdr4, hdr_small):
        """The helioprojective part of the 4-D header in degrees, not rounded (what map_builder.py:253-280 evaluates
        the slit positions with); CRVAL / CROTA come from the flattened header inside the library (the *_ref values)."""
        lon, lat = spice_header._axes(hdr4)
        s1 = hdrutil.unit_to_deg(str(hdr4.get("CUNIT%d" % lon, "deg")).strip() or "deg")
        s2 = hdrutil.unit_to_deg(str(hdr4.get("CUNIT%d" % lat, "deg")).strip() or "deg")
        t = {"NAXIS1": int(hdr_small["NAXIS1"]), "NAXIS2": int(hdr_small["NAXIS2"]),
             "CRPIX1": float(hdr4.get("CRPIX%d" % lon, 0.0)), "CRPIX2": float(hdr4.get("CRPIX%d" % lat, 0.0)),
             "CRVAL1": float(hdr4.get("CRVAL%d" % lon, 0.0)) * s1, "CRVAL2": float(hdr4.get("CRVAL%d" % lat, 0.0)) * s2,
             "CDELT1": float(hdr4.get("CDELT%d" % lon, 1.0)) * s1, "CDELT2": float(hdr4.get("CDELT%d" % lat, 1.0)) * s2,
             "CUNIT1": "deg", "CUNIT2": "deg", "CTYPE1": "HPLN-TAN", "CTYPE2": "HPLT-TAN",
             "LONPOLE": float(hdr4.get("LONPOLE", 180.0)), "CROTA": float(hdr_small.get("CROTA", 0.0))}
        for i, a in ((1, lon), (2, lat)):
            for j, b in ((1, lon), (2, lat)):
                t[f"PC{i}_{j}"] = float(hdr4.get(f"PC{a}_{b}", 1.0 if a == b else 0.0))
        return t

    def align_using_helioprojective(self, method="correlation", index_amplitude=None, extend_pixel_size=False):
        """alignment_spice.py:437-465."""
        self.lonlims = self.latlims = self.shape = self.reference_date = None
        self.method = method
        self.coordinate_frame = "final_helioprojective"
        self.extend_pixel_size = extend_pixel_size
        level = self._level()
        if level == 3 and self.despike_planes is not None:
            raise ValueError("despike_planes: a level-3 map has no wavelength planes to despike (level 2 only)")
        if level == 3:
            raise NotImplementedError("AlignementSpiceIterativeContextRaster: level-3 input (the reference's L3 path "
                                      "never sets the unflattened header it composes the context from)")
        # every imager file once: header and (memory-mapped / compressed) pixels
        loaded = [(fits_io.load_for_upload if self.raw_fits_upload else fits_io.read_image)(p, self.large_fov_window)
                  for p in self.large_fov_list_paths]
        headers = [fits_io.Header(h) for _, h in loaded]
        self.hdr_large = headers[0]  # (WAVELNTH for extend_pixel_size, _correct_solar_rotation)
        self._extract_spice_data_header(level=level, coeff=index_amplitude)
        hdr4 = self.header_spice_unflattened
        self.col_frame = self._frame_of_columns(hdr4, headers)
        used = sorted(set(int(i) for i in self.col_frame))
        col_slot = np.searchsorted(np.asarray(used), self.col_frame).astype(np.int32)
        frame_headers = []
        for i in used:
            hw = headers[i].copy()
            hdrutil.check_and_create_pcij_matrix(hw, False, warn=False)
            frame_headers.append(hw)
        # the composed header: the imager header of the middle column, SPICE pointing on top (map_builder.py:133-153)
        self.hdr_large = headers[int(self.col_frame[len(self.col_frame) // 2])]
        self._set_initial_header_values(True)
        if self.unit_lag != self.hdr_small["CUNIT1"]:
            raise ValueError("lag.unit and cUNIT are not the same")
        m = library_method(self.method)
        device = -1 if self.device is None else self.device
        h = _lib.shared_handle(device, self._handle_slot)
        h.reference_tag = None  # (the frames and the SPICE image replace whatever the handle held)
        frames = [fits_io.native_pixels(loaded[i][0]) if not isinstance(loaded[i][0], (fits_io.RawImage,
                                                                                    fits_io.CompressedImage))
                  else loaded[i][0] for i in used]
        h.set_context_frames(frames, frame_headers)
        h.set_small(np.asarray(self.data_small, dtype=np.float64))
        lags = _lib.LagSet(self.lag_crval1, self.lag_crval2, self.lag_cdelt1, self.lag_cdelt2, self.lag_crota)
        sem = _lib.CDELT_INTENDED if self.cdelt_semantics == "intended" else _lib.CDELT_REFERENCE
        target = self._celestial_degrees(hdr4, self.hdr_small)
        corr = h.sweep_context(target, self.hdr_small, col_slot, lags, order=self.order, method=m,
                               cdelt_semantics=sem, vmin=self.small_fov_value_min, vmax=self.small_fov_value_max)
        self.last_stats = h.last_stats()
        results = np.asarray(corr).reshape(lags.shape + (1,))
        self.last_counts = h.last_counts().reshape(results.shape)
        results = apply_min_overlap(results, self.last_counts, self.min_overlap)
        return self._wrap(results, "AlignmentResults", restore_units=True)
