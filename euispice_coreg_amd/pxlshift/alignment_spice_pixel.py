"""
`AlignmentSpicePixel` -- drop-in for euispice_coreg.pxlshift.AlignmentSpicePixel
(pxlshift/alignment_spice_pixel.py:9-101): the small image is a SPICE L2 window summed over wavelength between the
slit edges, with a 2-D header in degrees whose CDELT1 is shortened by the apparent solar rotation during one raster
step; the sweep is `AlignmentPixels.find_best_parameters`.  Level-3 input raises NotImplementedError.

Beyond the reference: `row_offset`, the first row of the L2 window that the small image holds, and
`write_destretched_fits`, the L2 file with the planes of the chosen windows resampled by a `LocalShiftField`; and
`despike_planes=` (`utils.despiking.despike_planes_params`): every wavelength plane is despiked on its own on the GPU over
the rows [ylim, ylen - ylim) and the planes are summed there (include/coreg_hip.h: coreg_despike_sum_planes_be) in place of
the host nansum; `last_despiked_planes` holds the flag events per pass, `despiked_plane_events` their int32 map on the small
image's grid.
"""
from __future__ import annotations

import numpy as np

from ..utils import fits_io, header as hdrutil, spice_header
from ..utils.despiking import despike_planes_params
from .alignment_pixels import AlignmentPixels, large_fov_centre, set_pixels_shift_cards


class AlignmentSpicePixel(AlignmentPixels):

    def __init__(self, fsi_path, fsi_window, spice_path, spice_window, index_amplitude=None, device=None,
                 despike_planes=None):
        self.despike_planes = despike_planes_params(despike_planes, "despike_planes")
        self.last_despiked_planes = self.despiked_plane_events = None
        self.fsi_path, self.spice_path = fsi_path, spice_path
        self.fsi_window, self.spice_window = fsi_window, spice_window
        name = spice_path if isinstance(spice_path, str) else ""
        if "L2" in name:
            level = 2
        elif "L3" in name:
            raise NotImplementedError("AlignmentSpicePixel: level-3 input is not implemented (the pixel-lag sweep takes "
                                      "SPICE L2 windows)")
        else:
            raise ValueError("the SPICE level is read from the file name: it must contain 'L2'")
        data, hdr = fits_io.read_image(fsi_path, fsi_window)
        self.hdr_large = fits_io.Header(hdr).copy()
        self.data_large = np.array(fits_io.native_pixels(data), dtype=np.float64)
        self.large_fov_known_pointing, self.window_large = fsi_path, fsi_window
        self.small_fov_to_correct, self.window_small = spice_path, spice_window
        self.device = device
        self.slc_small_ref = None
        self.ratio_res_1 = self.ratio_res_2 = None
        self.last_timing = None
        self.last_counts = None
        self._extract_spice_data_header(level=level, index_amplitude=index_amplitude)

    def _extract_spice_data_header(self, level, index_amplitude=None):
        """alignment_spice_pixel.py:29-45."""
        cube, hdr = fits_io.open_cube(self.spice_path, self.spice_window)
        hdr = fits_io.Header(hdr)
        dt = hdr["PC4_1"]
        self._prepare_spice_from_l2(cube, hdr)
        for k in ("SOLAR_B0", "RSUN_REF", "DSUN_OBS"):
            self.hdr_small[k] = hdr[k]
        self._correct_solar_rotation(dt)

    def _correct_solar_rotation(self, dt):
        """alignment_spice_pixel.py:47-62: CDELT1 -= dt * (apparent rotation rate), with the SPICE header's own B0,
        RSUN_REF and DSUN_OBS."""
        h = self.hdr_small
        B0 = np.deg2rad(h["SOLAR_B0"])
        band = self.hdr_large["WAVELNTH"]
        omega_car = np.deg2rad(360 / 25.38 / 86400)
        if band == 174:
            band = 171
        omega = omega_car + spice_header.diff_rot(B0, f"EIT {band}")
        Rsun, Dsun = h["RSUN_REF"], h["DSUN_OBS"]
        phi = np.rad2deg(omega * Rsun / (Dsun - Rsun)) * 3600  # arcsec / s
        h["CDELT1"] = float(h["CDELT1"] - hdrutil.convert(dt * phi, "arcsec", h["CUNIT1"]))

    def _prepare_spice_from_l2(self, cube, hdr):
        """alignment_spice_pixel.py:64-86."""
        cube = np.asarray(cube)
        if cube.ndim != 4:
            raise ValueError("a SPICE L2 window is a 4-D cube [time, wavelength, y, x]")
        ymin, ymax = spice_header.vertical_edges_limits(hdr)
        self.hdr_small = spice_header.celestial_header(hdr)
        ylen = cube.shape[2]
        ylim = max(ymin, ylen - ymax - 1)
        self.row_offset = int(ylim)  # row 0 of the small image is row `row_offset` of the window
        # (a reduction over the outer axis adds the planes one after another, as the reference's nansum does)
        if self.despike_planes is not None:
            from ..hdrshift.alignment_spice import despiked_plane_sum
            r0, r1, _ = slice(ylim, ylen - ylim).indices(ylen)
            image, events, self.last_despiked_planes = despiked_plane_sum(
                cube[0], np.arange(cube.shape[1]), self.despike_planes, (r0, max(r0, r1)), self.device)
            self.data_small, self.despiked_plane_events = image[r0:max(r0, r1)], events[r0:max(r0, r1)]
        else:
            self.data_small = np.nansum(np.asarray(cube[0][:, ylim:(ylen - ylim), :], dtype=np.float64), axis=0)
        self.hdr_small["CRPIX1"] = (self.data_small.shape[1] + 1) / 2
        self.hdr_small["CRPIX2"] = (self.data_small.shape[0] + 1) / 2
        self.hdr_small["NAXIS1"] = self.data_small.shape[1]
        self.hdr_small["NAXIS2"] = self.data_small.shape[0]

    def write_destretched_fits(self, field, windows, path_out, reference=None):
        """Write every HDU of the L2 file to `path_out`; in the windows named in `windows` (EXTNAME, index or index from
        the end, as `write_corrected_fits` selects them) every plane of `cube[0]` is destretched by `field` (a
        `LocalShiftField` of this object's `find_local_shifts`) about the rigid shift `reference` = (rx, ry), default the
        field's `median_shift`, and the header gets the four cards of `align_pixels_shift` at that shift plus DSTRETCH
        (True), DSTR_DX and DSTR_DY (the reference, pixels).  ValueError for a window whose (ny, nx) is not that of the
        window the field was measured on, and when no window is selected."""
        rx, ry = field._reference(reference)
        want = (field.image_shape[0] + 2 * self.row_offset, field.image_shape[1])
        hdus = fits_io.read_all(self.spice_path)
        mid = None
        out, n = [], len(hdus)
        for ii, (data, hdr) in enumerate(hdus):
            if not ((hdr.get("EXTNAME", "nothing98695") in windows) or (ii in windows) or ((ii - n) in windows)):
                out.append((data, hdr))
                continue
            if data is None or np.ndim(data) != 4 or tuple(np.shape(data)[2:]) != want:
                raise ValueError(f"window {ii}: a cube [time, wavelength, {want[0]}, {want[1]}] is needed, the shape of "
                                 "the window the field was measured on")
            if mid is None:
                mid = large_fov_centre(self.fsi_path, self.fsi_window)
            data = np.array(data)
            data[0] = field.destretch(data[0], reference=(rx, ry), row_offset=self.row_offset, device=self.device)
            hdr = fits_io.Header(hdr).copy()
            set_pixels_shift_cards(hdr, mid, rx, ry)
            hdr["DSTRETCH"], hdr["DSTR_DX"], hdr["DSTR_DY"] = True, float(rx), float(ry)
            out.append((data, hdr))
        if mid is None:
            raise ValueError("has not corrected any window.")
        fits_io.write_images(path_out, out)
