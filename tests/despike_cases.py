"""
What tests/test_gpu_despike.py and tests/test_gpu_despike_planes.py share: the kernel's tile (read from
csrc/despike_plan.hpp), the rule with a min_neighbours that fits the shape, and the seeded pixels -- `stack` makes n planes,
`image` is its single plane.
"""
import os
import re

import numpy as np

_PLAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "euispice_coreg_amd", "csrc", "despike_plan.hpp")


def _plan_constant(name):
    with open(_PLAN) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


TILE_H, TILE_W = _plan_constant("kDespikeTileH"), _plan_constant("kDespikeTileW")


def stack(n, shape, seed, dtype, kind="noise"):
    """n planes about 100 with unit noise, a spike on every 11th pixel or so (some of them side by side) and a few negative
    ones, each plane with its own; float64 values are not float32-exact (they stay float64 on the device).  kind
    "integers": ties and half-integer medians; "constant": 7 everywhere."""
    rng = np.random.default_rng(seed)
    full = (n,) + tuple(shape)
    if kind == "integers":
        v = rng.integers(0, 4, full).astype(np.float64)
        v[rng.uniform(size=full) < 0.08] += 40.0
        return v.astype(dtype)
    if kind == "constant":
        return np.full(full, 7.0, dtype=dtype)
    v = 100.0 + rng.normal(0.0, 1.0, full)
    hit = rng.uniform(size=full) < 0.09
    v[hit] += rng.uniform(20.0, 4000.0, int(hit.sum()))
    v[rng.uniform(size=full) < 0.03] -= 60.0  # negative spikes: sign = both sees them
    if dtype == np.float32:
        return v.astype(np.float32)
    v = v + 1e-9 * np.pi
    assert not np.array_equal(v, v.astype(np.float32).astype(np.float64))
    return v


def image(shape, seed, dtype, kind="noise"):
    """One plane of `stack`: the same seed gives the pixels of stack(1, ...)[0]."""
    return stack(1, shape, seed, dtype, kind)[0]


def rule(R, n_iter, shape=(99, 99), **kw):
    """min_neighbours 5, or as many as an interior pixel of an image of `shape` has when that is fewer."""
    most = min(shape[0], 2 * R + 1) * min(shape[1], 2 * R + 1) - 1
    return dict(radius=R, n_iter=n_iter, min_neighbours=max(1, min(5, most)), **kw)
