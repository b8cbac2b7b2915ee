"""
Differential rotation of the Carrington resamples (utils/rectify.py:282-311, :416-423 of the reference): which band a
reference image selects, its rotation-rate coefficients, and the time difference the rotation is applied over.

The reference builds this transform for every Carrington resample but looks its band up with an integer WAVELNTH in a
table with string keys (hdrshift/alignment.py:107-108, :891-894): the lookup never matches and the coefficients cancel
(quirk Q5).  `Alignment(differential_rotation="intended")` applies the arithmetic the reference holds.
"""
from __future__ import annotations

import datetime as _dt

from .spice_header import parse_date

# hdrshift/alignment.py:107-108 (keys as the integers the header holds)
BAND_OF_WAVELENGTH = {171: "171", 193: "195", 211: "195", 131: "171", 304: "304", 335: "304", 94: "171", 174: "171"}
# utils/rectify.py:293-300: degrees / day, A + B sin^2(lat) + C sin^4(lat)
RATE_COEFFICIENTS = {"171": (14.56, -2.65, 0.96), "195": (14.50, -2.14, 0.66), "284": (14.60, -0.71, -1.18),
                     "304": (14.51, -3.12, 0.34)}


def rotation_band(hdr_large):
    """The band ('171', '195', '304') the reference image's WAVELNTH selects -- for both images of an alignment
    (alignment.py:891) -- or None: no WAVELNTH card, a value that is not a whole number, or one outside the table."""
    w = hdr_large.get("WAVELNTH") if hasattr(hdr_large, "get") else None
    try:
        w = float(w)
    except (TypeError, ValueError):
        return None
    if w != w or w != int(w):
        return None
    return BAND_OF_WAVELENGTH.get(int(w))


def _as_datetime(date):
    if isinstance(date, _dt.datetime):
        return date.replace(tzinfo=None)
    if hasattr(date, "isot"):  # astropy.time.Time
        date = date.isot
    return parse_date(date)


def delta_t_days(date_obs, reference_date) -> float:
    """(date_obs - reference_date) in days, rectify.py:418.  Calendar arithmetic: leap seconds inside the interval are
    ignored (astropy's UTC difference counts them: 1.2e-5 d each, 1.7e-4 degrees of rotation at most)."""
    return (_as_datetime(date_obs) - _as_datetime(reference_date)) / _dt.timedelta(days=1)


def rotation(hdr, hdr_large, reference_date):
    """(delta_t_days, c0, c1, c2) of the Carrington resample of the image `hdr` describes, or None when nothing
    rotates: no reference date (rectify.py:416-417: the image's own DATE-OBS, delta_t = 0) or no band.  KeyError when
    `hdr` has no DATE-OBS, as the reference raises."""
    if reference_date is None:
        return None
    band = rotation_band(hdr_large)
    if band is None:
        return None
    if "DATE-OBS" not in hdr:
        raise KeyError("DATE-OBS")
    return (delta_t_days(hdr["DATE-OBS"], reference_date),) + RATE_COEFFICIENTS[band]
