#!/usr/bin/env python3
"""
Timing of the pixel-lag sweep (pxlshift.AlignmentPixels) on a SPICE-like workload: an 832 x 192 raster against a
3072 x 3072 image, ratios (0.94, 0.247), 61 x 61 x 21 lags (1.25e10 pixel pairs per pass), synthetic data.

Measured warm (one call first, then `--repeat` timed calls, the median reported):
  * the whole `find_best_parameters` call, wall clock around the call (it returns with the cube in host memory);
  * preparation (sub-resolved box + rotation planes), pass 0 and pass 1 of the sweep kernel, between HIP events the
    library records on its stream (coreg_pixels_last_timing).
Baseline: tests/pxlshift_oracle.py (numpy, one lag at a time as the reference walks them) on every 100th lag on this
machine's CPU, times 100, plus its 21 rotation planes.

    python profiles/pxlshift_timing.py [--out profiles/pxlshift_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from euispice_coreg_amd import synthetic  # noqa: E402
from euispice_coreg_amd.pxlshift import AlignmentPixels  # noqa: E402
from tests import pxlshift_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--large-n", type=int, default=3072)
    ap.add_argument("--half", type=int, default=30, help="dx, dy in [-half, half]")
    ap.add_argument("--n-rot", type=int, default=21)
    a = ap.parse_args()

    lcd = 4.44 * 3072 / a.large_n
    small, hs, large, hl, _ = synthetic.make_scene(small_shape=tuple(a.small), large_n=a.large_n, n_blobs=300,
                                                   small_cdelt=(0.94 * lcd, 0.247 * lcd), large_crval=(-310.0, 420.0))
    A = AlignmentPixels((large, hl), 0, (small, hs), 0)
    lag_dx = lag_dy = np.arange(-a.half, a.half + 1)
    lag_drot = np.linspace(-1.0, 1.0, a.n_rot)
    corr = A.find_best_parameters(lag_dx, lag_dy, lag_drot)  # warm-up
    calls, prep, p0, p1 = [], [], [], []
    for _ in range(a.repeat):
        t = time.perf_counter()
        again = A.find_best_parameters(lag_dx, lag_dy, lag_drot)
        calls.append(time.perf_counter() - t)
        prep.append(A.last_timing["prepare_ms"])
        p0.append(A.last_timing["pass0_ms"])
        p1.append(A.last_timing["pass1_ms"])
    assert np.array_equal(again, corr, equal_nan=True)
    pairs = float(small.size) * corr.size

    # CPU baseline: the box the lags can reach, the planes, every 100th lag
    h, w = small.shape
    l = A._last_plan["slc_small_ref"]
    t = time.perf_counter()
    x, y = np.meshgrid(np.arange(l[1] - a.half, l[1] + w + a.half) * A.ratio_res_1,
                       np.arange(l[0] - a.half, l[0] + h + a.half) * A.ratio_res_2)
    box = O.fill_to_nan(O.interpol2d(large, x, y, -32768), -32768)
    t_box = time.perf_counter() - t
    t = time.perf_counter()
    planes = [O.rotate(small, d, "degree") for d in lag_drot]
    t_planes = time.perf_counter() - t
    idx = np.arange(0, corr.size, 100)
    worst = 0.0
    t = time.perf_counter()
    for q in idx:
        i, j, k = np.unravel_index(q, corr.shape)
        r0, c0 = a.half + lag_dy[j], a.half + lag_dx[i]
        v = O.correlate(box[r0:r0 + h, c0:c0 + w], planes[k])
        worst = max(worst, abs(v - corr[i, j, k]))
    t_lags = time.perf_counter() - t
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {"workload": {"small": list(small.shape), "large": list(large.shape), "ratios": [A.ratio_res_1, A.ratio_res_2],
                        "lags": list(corr.shape), "pixel_pairs_per_pass": pairs},
           "gpu": {"call_s": med(calls), "prepare_ms": med(prep), "pass0_ms": med(p0), "pass1_ms": med(p1),
                   "pass0_pairs_per_s": pairs / (med(p0) * 1e-3), "pass1_pairs_per_s": pairs / (med(p1) * 1e-3),
                   "repeat": a.repeat, "calls_s": calls},
           "cpu_oracle": {"sampled_lags": int(idx.size), "sampled_s": t_lags, "planes_s": t_planes, "box_s": t_box,
                          "extrapolated_sweep_s": t_lags * corr.size / idx.size + t_planes,
                          "max_abs_diff_to_gpu_on_sample": worst},
           "argmax": [int(v) for v in np.unravel_index(np.nanargmax(corr), corr.shape)]}
    res["speedup_sweep_vs_cpu_oracle"] = res["cpu_oracle"]["extrapolated_sweep_s"] / res["gpu"]["call_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
