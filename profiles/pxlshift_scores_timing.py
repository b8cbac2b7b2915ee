#!/usr/bin/env python3
"""
Pass times of the pixel-lag sweep (pxlshift.AlignmentPixels) per score on the README's workload shape: an 832 x 192
raster against a 3072 x 3072 image, ratios (0.94, 0.247), 61 x 61 x 21 lags (1.25e10 pixel pairs per pass), synthetic
data (the scene of profiles/pxlshift_timing.py).

Each method runs in a child process of its own under a time limit: one warm-up call, then `--repeat` timed calls; the
library's HIP-event times (coreg_pixels_last_timing: preparation, first pass, second pass) are reported as medians with
every sample kept, next to the wall clock of the call and the count range of the cube.

    python profiles/pxlshift_scores_timing.py [--out profiles/pxlshift_scores_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("correlation", "residus_masked")


def run_method(a):
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    lcd = 4.44 * 3072 / a.large_n
    small, hs, large, hl, _ = synthetic.make_scene(small_shape=tuple(a.small), large_n=a.large_n, n_blobs=300,
                                                   small_cdelt=(0.94 * lcd, 0.247 * lcd), large_crval=(-310.0, 420.0))
    A = AlignmentPixels((large, hl), 0, (small, hs), 0)
    lag_dx = lag_dy = np.arange(-a.half, a.half + 1)
    lag_drot = np.linspace(-1.0, 1.0, a.n_rot)
    cube = A.find_best_parameters(lag_dx, lag_dy, lag_drot, method=a.method)  # warm-up
    calls, t = [], {"prepare_ms": [], "pass0_ms": [], "pass1_ms": []}
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        again = A.find_best_parameters(lag_dx, lag_dy, lag_drot, method=a.method)
        calls.append(time.perf_counter() - t0)
        for k in t:
            t[k].append(A.last_timing[k])
    assert np.array_equal(again, cube, equal_nan=True)
    best = (np.nanargmin if a.method == "residus_masked" else np.nanargmax)(cube)
    res = {"method": a.method, "call_s": float(np.median(calls)), "calls_s": calls,
           "best_index": [int(v) for v in np.unravel_index(best, cube.shape)], "n_nan": int(np.isnan(cube).sum()),
           "counts": [float(A.last_counts.min()), float(A.last_counts.max())],
           "workload": {"small": list(small.shape), "large": list(large.shape), "lags": list(cube.shape),
                        "ratios": [A.ratio_res_1, A.ratio_res_2], "pixel_pairs_per_pass": float(small.size) * cube.size}}
    for k, v in t.items():
        res[k] = float(np.median(v))
        res[k + "_samples"] = v
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_scores_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--large-n", type=int, default=3072)
    ap.add_argument("--half", type=int, default=30, help="dx, dy in [-half, half]")
    ap.add_argument("--n-rot", type=int, default=21)
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one method's child process [s]")
    ap.add_argument("--method", choices=METHODS, help="(child) run this method in this process")
    a = ap.parse_args()
    if a.method:
        return run_method(a)
    out = {}
    for m in METHODS:
        cmd = [sys.executable, os.path.abspath(__file__), "--method", m, "--repeat", str(a.repeat), "--small",
               str(a.small[0]), str(a.small[1]), "--large-n", str(a.large_n), "--half", str(a.half), "--n-rot", str(a.n_rot)]
        r = subprocess.run(cmd, timeout=a.limit, check=True, capture_output=True, text=True)  # (a failure ends the run)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out[m] = json.loads(line[len("RESULT "):])
    res = {"workload": out[METHODS[0]].pop("workload"), "methods": out}
    out[METHODS[1]].pop("workload")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
