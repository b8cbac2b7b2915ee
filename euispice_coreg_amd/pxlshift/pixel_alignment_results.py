"""
`PixelAlignmentResults` -- what `AlignmentPixels.find_best_parameters(..., return_type="PixelAlignmentResults")` returns:
the cube of the integer pixel-lag sweep with its lag axes, the sample count behind every entry, the best entry
(maximum of a correlation or of `mutual_information`, minimum of `residus_masked`) and its sub-lag position on the
(dx, dy) plane of the best rotation -- the Gaussian fit `hdrshift.AlignmentResults` runs (`hdrshift.alignment_results.gaussian_sub_lag`: quirk Q13's
neighbours, start, bounds, native / scipy, the flipped rescaled plane for a minimum, the fall-back to the best entry).
The shift goes into a header through `align_pixels_shift`, which takes fractional pixels; the best rotation is
reported (`drot`), not written: `align_pixels_shift` has no rotation, as in the reference.
"""
from __future__ import annotations

import os

import numpy as np

from ..hdrshift.alignment_results import gaussian_sub_lag
from ..utils import fits_io
from .alignment_pixels import align_pixels_shift, large_fov_centre, set_pixels_shift_cards

_BEST = {"correlation": "max", "residus_masked": "min", "mutual_information": "max"}


class PixelAlignmentResults:

    def __init__(self, corr, lag_dx, lag_dy, lag_drot, unit_rot="degree", method="correlation", n_samples=None,
                 large_fov_path=None, large_fov_window=None, small_fov_path=None, fit=None):
        if method not in _BEST:
            raise NotImplementedError
        fit = fit or os.environ.get("COREG_GAUSSIAN_FIT", "native")
        if fit not in ("native", "scipy"):
            raise ValueError("fit must be 'native' or 'scipy'")
        self.fit = fit
        self.method = method
        self.best = _BEST[method]
        corr = np.asarray(corr)
        self.lag_dx, self.lag_dy, self.lag_drot = (np.atleast_1d(np.asarray(v)) for v in (lag_dx, lag_dy, lag_drot))
        if corr.shape != (len(self.lag_dx), len(self.lag_dy), len(self.lag_drot)):
            raise ValueError("corr must be shaped [len(lag_dx), len(lag_dy), len(lag_drot)]")
        self.corr = corr
        self.n_samples = n_samples
        self.unit_rot = unit_rot
        self.large_fov_path, self.large_fov_window = large_fov_path, large_fov_window
        self.small_fov_path = small_fov_path
        # (an all-NaN cube raises numpy's ValueError here)
        self.max_index = np.unravel_index((np.nanargmin if self.best == "min" else np.nanargmax)(corr), corr.shape)
        mi = self.max_index
        pos, self.fit_info = gaussian_sub_lag(corr[:, :, mi[2]], (mi[0], mi[1]), self.best, fit)
        self.fitted = pos is not None
        self.shift_index = (mi[0], mi[1]) if pos is None else (pos[0], pos[1])
        x, y = self.shift_index
        self.shift_pixels = (np.interp(x, np.arange(len(self.lag_dx)), self.lag_dx),
                             np.interp(y, np.arange(len(self.lag_dy)), self.lag_dy))
        self.drot = self.lag_drot[mi[2]]

    def _paths(self):
        if self.large_fov_path is None or self.small_fov_path is None:
            raise ValueError("the paths of both images are needed (a PixelAlignmentResults built by AlignmentPixels has them)")
        return self.large_fov_path, self.large_fov_window, self.small_fov_path

    def return_corrected_header(self, windows):
        """`align_pixels_shift` at the sub-lag shift: the header of the last window of `windows`."""
        large, window, small = self._paths()
        return align_pixels_shift(self.shift_pixels[0], self.shift_pixels[1], windows, large, window, small)

    def write_corrected_fits(self, windows, path_out):
        """Copy the small image's file with the four cards of `align_pixels_shift` set in every HDU named in `windows`
        (EXTNAME, index or index from the end), as `AlignmentResults.write_corrected_fits` copies and selects them."""
        large, window, small = self._paths()
        mid = large_fov_centre(large, window)

        def selected(ii, n, hdr):
            return (hdr.get("EXTNAME", "nothing98695") in windows) or (ii in windows) or ((ii - n) in windows)

        def correct(hdr):
            set_pixels_shift_cards(hdr, mid, self.shift_pixels[0], self.shift_pixels[1])
        if fits_io.rewrite_with_corrected_headers(small, path_out, selected, correct) == 0:
            raise ValueError("has not corrected any window.")

    def __str__(self):
        return (f"\n Shift : \n dx = {self.shift_pixels[0]} pixels \n dy = {self.shift_pixels[1]} pixels "
                f"\n drot = {self.drot} {self.unit_rot} ({self.method}, best = {self.best})")

    __repr__ = __str__
