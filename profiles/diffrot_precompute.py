#!/usr/bin/env python3
"""precompute_ms (coreg_stats: the k_precompute / k_tile_list launches of one sweep) with differential rotation off and
on, at the headline shape (2048^2 grid, 60 x 60 CRVAL lags, 1 launch) and at cfg5's (4096^2 grid, 41 x 41 x 5 x 5 x 11
lags, 275 launches).  With rotation on, every k_precompute launch forms lon' per grid point and takes a float64 sincos
(no cached [gh][gw] sin / cos pair).  Writes profiles/diffrot_precompute.json.
usage: python profiles/diffrot_precompute.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from euispice_coreg_amd import _lib, synthetic  # noqa: E402

ROT = (0.25, 14.51, -3.12, 0.34)  # 6 h, band 304


def measure(h, hs, large, hl, shape, lag_arrays, reps):
    grid = _lib.Grid((200, 300), (-20, 20), shape)
    lags = _lib.LagSet(*lag_arrays)
    out = {}
    for name, rot in (("off", None), ("on", ROT)):
        h.set_rotation("reference", rot)
        h.set_rotation("small", rot)
        h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        best = None
        for _ in range(reps + 1):  # first run: warm-up
            h.sweep_carrington(hs, grid, 1.004, lags)
            st = h.last_stats()
            if best is None or st["precompute_ms"] < best["precompute_ms"]:
                best = st
        out[name] = dict(precompute_ms=best["precompute_ms"], sweep_kernel_ms=best["sweep_kernel_ms"],
                         total_gpu_ms=best["total_gpu_ms"], launches=best["n_sweep_launches"],
                         active_points=best["n_active_points"])
    h.set_rotation("reference", None)
    h.set_rotation("small", None)
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "diffrot_precompute.json")
    h = _lib.CoregHandle(0)
    small, hs, large, hl, _ = synthetic.make_scene()
    h.set_small(small)
    res = {"rotation": dict(zip(("delta_t_days", "c0", "c1", "c2"), ROT)),
           "headline": measure(h, hs, large, hl, (2048, 2048),
                               (np.arange(-30, 30, 1.0), np.arange(-30, 30, 1.0), None, None, None), reps=5),
           "cfg5": measure(h, hs, large, hl, (4096, 4096),
                           (np.arange(-20, 21, 1.0), np.arange(-20, 21, 1.0), np.round(np.arange(-2, 3) * 0.01, 10),
                            np.round(np.arange(-2, 3) * 0.01, 10), np.round(np.arange(-5, 6) * 0.1, 10)), reps=1)}
    with open(dst, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
