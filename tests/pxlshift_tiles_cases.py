"""Scenes of the local-shift-field tests (shared by the CPU and the GPU tests)."""
import numpy as np

from . import pxlshift_oracle as O

HDR = {"CDELT1": 1.0, "CDELT2": 1.0, "CUNIT1": "arcsec", "CUNIT2": "arcsec"}


def two_drift_scene():
    """A 40 x 48 small image whose left half (columns 0-23) lies at (dx, dy) = (2, -1) of a 70 x 86 large image and whose
    right half at (-1, 2): no single lag fits it.  Returns (large, small, keyword arguments of the sweep, tile shape,
    expected (dx, dy) per tile [2][2])."""
    rng = np.random.default_rng(31)
    raw = rng.uniform(1.0, 9.0, (70, 86))
    # 3 x 3 box mean, edges by wrap-around: structure wider than a pixel, values still in (1, 9)
    large = sum(np.roll(np.roll(raw, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    h, w = 40, 48
    l = O.slice_origin(large.shape, (h, w))
    small = np.empty((h, w))
    halves = ((slice(0, 24), (2, -1)), (slice(24, 48), (-1, 2)))
    for cols, (dx, dy) in halves:
        small[:, cols] = large[l[0] + dy:l[0] + dy + h, l[1] + dx + cols.start:l[1] + dx + cols.stop]
    small += rng.normal(0, 0.02, small.shape)
    small[rng.integers(0, h, 25), rng.integers(0, w, 25)] = np.nan
    large[rng.integers(0, 70, 40), rng.integers(0, 86, 40)] = np.nan
    kw = dict(lag_dx=np.arange(-4, 5), lag_dy=np.arange(-4, 5), lag_drot=np.array([0.0]))
    want = [[halves[0][1], halves[1][1]], [halves[0][1], halves[1][1]]]
    return large, small, kw, (20, 24), want


def two_drift_object():
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    large, small, kw, tile_shape, want = two_drift_scene()
    return AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0), kw, tile_shape, want
