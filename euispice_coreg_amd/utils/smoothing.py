"""
The weight tables of the NaN-aware smoothing (include/coreg_hip.h: coreg_smooth_small): what a
`smooth_small=` / `smooth_large=` keyword becomes before it reaches the library.  numpy only.
"""
from __future__ import annotations

import math

import numpy as np

MAX_R = 64  # csrc/smooth_plan.hpp: kSmoothMaxR
_FWHM_TO_SIGMA = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))


def gaussian_table(fwhm, what="smoothing"):
    """The table of one axis of a Gaussian of full width at half maximum `fwhm` [pixels]: sigma = fwhm / (2 sqrt(2 ln 2)),
    r = ceil(4 sigma), w[k] = exp(-(k - r)^2 / (2 sigma^2)) / sum; fwhm = 0 is the identity [1.0]; r > 64: ValueError."""
    fwhm = float(fwhm)
    if not (math.isfinite(fwhm) and fwhm >= 0):
        raise ValueError(f"{what}: a FWHM must be a finite number >= 0 (got {fwhm})")
    if fwhm == 0:
        return np.ones(1, dtype=np.float64)
    sigma = fwhm * _FWHM_TO_SIGMA
    r = int(math.ceil(4.0 * sigma))
    if r > MAX_R:
        raise ValueError(f"{what}: a FWHM of {fwhm} pixels needs taps out to r = {r} pixels, more than the {MAX_R} a "
                         "smoothing table can reach")
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * sigma * sigma))
    return w / w.sum()


def check_table(t, what="smoothing"):
    """A table as the library takes it: 1-D, an odd number of entries from 1 to 129, finite, >= 0, positive sum."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    if t.ndim != 1 or not 1 <= t.size <= 2 * MAX_R + 1 or t.size % 2 == 0:
        raise ValueError(f"{what}: a table needs an odd number of entries from 1 to {2 * MAX_R + 1}")
    if not (np.all(np.isfinite(t)) and np.all(t >= 0) and t.sum() > 0):
        raise ValueError(f"{what}: the entries of a table must be finite, >= 0 and have a positive sum")
    return t.copy()


def smoothing_tables(arg, what="smoothing", scale=(1.0, 1.0)):
    """(wy, wx), float64 tables, of a smoothing argument; None for None.  A number: the FWHM of a Gaussian on both axes; a
    pair of numbers: (fwhm_y, fwhm_x) (`gaussian_table`); a pair of 1-D arrays: the tables themselves (`check_table`).
    `scale` = (sy, sx) multiplies a FWHM before it is used (a unit conversion to pixels); tables are taken as they are."""
    if arg is None:
        return None
    err = ValueError(f"{what} must be None, a FWHM, a pair (fwhm_y, fwhm_x) or a pair of weight tables")
    if isinstance(arg, (bool, np.bool_, str)):
        raise err
    if isinstance(arg, (int, float, np.number)) or (isinstance(arg, np.ndarray) and arg.ndim == 0):
        arg = (arg, arg)
    try:
        ay, ax = arg
    except (TypeError, ValueError):
        raise err from None
    if any(isinstance(v, (bool, np.bool_, str)) for v in (ay, ax)):
        raise err
    if np.ndim(ay) == 0 and np.ndim(ax) == 0:
        try:
            fy, fx = float(ay) * float(scale[0]), float(ax) * float(scale[1])
        except (TypeError, ValueError):
            raise err from None
        return gaussian_table(fy, what), gaussian_table(fx, what)
    if np.ndim(ay) != 1 or np.ndim(ax) != 1:
        raise err
    return check_table(ay, what), check_table(ax, what)
