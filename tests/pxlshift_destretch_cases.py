"""Scenes of the destretch tests (shared by the CPU and the GPU tests)."""
import numpy as np

from . import pxlshift_oracle as O
from .pxlshift_tiles_cases import HDR


def smooth_drift_scene():
    """A 48 x 72 small image sampled from a 90 x 120 large image (the two-drift scene's recipe: a 3 x 3 box mean of
    uniform noise) at a shift that drifts smoothly across the columns: dx = -1.5 + 3 x / 71, dy = 1 - 2 x / 71, order 1,
    plus noise of 0.02 and 30 NaN pixels.  Returns (large, small, keyword arguments of the sweep, tile shape)."""
    rng = np.random.default_rng(7)
    raw = rng.uniform(1.0, 9.0, (90, 120))
    large = sum(np.roll(np.roll(raw, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    h, w = 48, 72
    l = O.slice_origin(large.shape, (h, w))
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dx, dy = -1.5 + 3.0 * x / 71.0, 1.0 - 2.0 * x / 71.0
    small = O.interpol2d(large, l[1] + x + dx, l[0] + y + dy, np.nan)
    small = small + rng.normal(0, 0.02, small.shape)
    small[rng.integers(0, h, 30), rng.integers(0, w, 30)] = np.nan
    kw = dict(lag_dx=np.arange(-4, 5), lag_dy=np.arange(-4, 5), lag_drot=np.array([0.0]))
    return large, small, kw, (24, 12)


def pair(large, small):
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    return AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0)
