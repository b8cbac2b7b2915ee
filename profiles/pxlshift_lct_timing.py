#!/usr/bin/env python3
"""
Pass times of the apodized windows of the local shift field (pxlshift.AlignmentPixels.find_local_shifts(tile_step=...,
apodization=...), k_pixels_lct) next to the unapodized passes on the same windows (k_pixels_sweep_tiles<0 / 1>), on the
workload of DESIGN section 9a: an 832 x 192 raster against a 3072 x 3072 image, ratios (0.94, 0.247), 61 x 61 lags, one
rotation, synthetic data; windows of (64, 64) at step (32, 32), 25 x 5 of them.

Both runs in one child process under a time limit, each one warm-up call and `--repeat` timed calls.  The library's
HIP-event times (coreg_pixels_last_timing: preparation, first pass, second pass) are reported as medians with every sample
kept, next to the wall clock of the call (`sub_lag=False`: cubes, counts and best entries, no fits), the disjoint tiles of
the same shape for scale, and the ratio of either apodized pass to the unapodized pass of the same windows.

    python profiles/pxlshift_lct_timing.py [--out profiles/pxlshift_lct_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPANS = ("prepare_ms", "pass0_ms", "pass1_ms")


def _timed(call, A, repeat):
    first = call()  # warm-up
    calls, t = [], {k: [] for k in SPANS}
    for _ in range(repeat):
        t0 = time.perf_counter()
        again = call()
        calls.append(time.perf_counter() - t0)
        for k in SPANS:
            t[k].append(A.last_timing[k])
    res = {"call_s": float(np.median(calls)), "calls_s": calls}
    for k, v in t.items():
        res[k] = float(np.median(v))
        res[k + "_samples"] = v
    return first, again, res


def run(a):
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    lcd = 4.44 * 3072 / a.large_n
    small, hs, large, hl, _ = synthetic.make_scene(small_shape=tuple(a.small), large_n=a.large_n, n_blobs=300,
                                                   small_cdelt=(0.94 * lcd, 0.247 * lcd), large_crval=(-310.0, 420.0))
    A = AlignmentPixels((large, hl), 0, (small, hs), 0)
    lag_dx = lag_dy = np.arange(-a.half, a.half + 1)
    lag_drot = np.array([0.0])
    tile, step = tuple(a.tile), tuple(a.step)
    runs = {}
    for label, kw in (("disjoint", {}), ("stepped", {"tile_step": step}),
                      ("apodized", {"tile_step": step, "apodization": "gaussian"})):
        F, G, res = _timed(lambda: A.find_local_shifts(lag_dx, lag_dy, lag_drot, tile_shape=tile, sub_lag=False, **kw), A,
                           a.repeat)
        assert np.array_equal(F.corr, G.corr, equal_nan=True)
        windows = F.valid.size
        res.update(tile_shape=list(tile), tile_step=list(F.tile_step), tile_grid=list(F.valid.shape),
                   n_valid=int(F.valid.sum()), median_shift=list(F.median_shift), scatter=list(F.scatter),
                   pixel_pairs_per_pass=float(sum((r.stop - r.start) * (c.stop - c.start) for row in F.tile_slices
                                                  for r, c in row)) * len(lag_dx) * len(lag_dy))
        res["pairs_per_s"] = [res["pixel_pairs_per_pass"] / (res[k] * 1e-3) for k in ("pass0_ms", "pass1_ms")]
        runs[label] = res
        if label == "stepped":
            counts = F.n_samples
        if label == "apodized":
            assert np.array_equal(F.n_samples, counts)  # the count of an entry stays the kept pixels
    for k in ("pass0", "pass1"):
        runs["apodized"][k + "_ratio"] = runs["apodized"][k + "_ms"] / runs["stepped"][k + "_ms"]
    plan = A._last_plan
    out = {"runs": runs, "workload": {"small": list(small.shape), "large": list(large.shape),
                                      "lags": [len(lag_dx), len(lag_dy), 1],
                                      "ratios": [plan["ratio_res_1"], plan["ratio_res_2"]], "windows": windows,
                                      "repeat": a.repeat}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_lct_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--tile", type=int, nargs=2, default=(64, 64))
    ap.add_argument("--step", type=int, nargs=2, default=(32, 32))
    ap.add_argument("--large-n", type=int, default=3072)
    ap.add_argument("--half", type=int, default=30, help="dx, dy in [-half, half]")
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of the child process [s]")
    ap.add_argument("--child", action="store_true", help="(child) run in this process")
    a = ap.parse_args()
    if a.child:
        return run(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--small", str(a.small[0]),
           str(a.small[1]), "--tile", str(a.tile[0]), str(a.tile[1]), "--step", str(a.step[0]), str(a.step[1]), "--large-n",
           str(a.large_n), "--half", str(a.half)]
    r = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
    if r.returncode != 0:  # (a failure ends the run)
        sys.exit(f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
