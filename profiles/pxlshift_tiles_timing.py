#!/usr/bin/env python3
"""
Pass times of the tiled pixel-lag sweep (pxlshift.AlignmentPixels.find_local_shifts) next to the untiled one of the same
run, per score, on the workload of profiles/pxlshift_scores_timing.py: an 832 x 192 raster against a 3072 x 3072 image,
ratios (0.94, 0.247), 61 x 61 x 21 lags (1.25e10 pixel pairs per pass), synthetic data.

Three runs per method, each one warm-up call and `--repeat` timed calls: the untiled `find_best_parameters`, tiles of
(64, 64) -- 13 x 3 tiles, bands of 64 x 32 pixels -- and one tile of the whole image (832, 192), the control: the walk
of the untiled call through the tiled kernel.  Each method runs in a child process of its own under a time limit.  The
library's HIP-event times (coreg_pixels_last_timing: preparation, first pass, second pass) are reported as medians with
every sample kept, next to the wall clock of the call (the tiled calls with `sub_lag=False`: cubes, counts and best
entries, no fits) and the ratio of either pass to the untiled pass of the same run.

    python profiles/pxlshift_tiles_timing.py [--out profiles/pxlshift_tiles_timing.json]
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
    cube, again, untiled = _timed(lambda: A.find_best_parameters(lag_dx, lag_dy, lag_drot, method=a.method), A, a.repeat)
    assert np.array_equal(again, cube, equal_nan=True)
    counts = A.last_counts
    runs = {"untiled": untiled}
    for label, ts in (("tiles_%dx%d" % tuple(a.tile), tuple(a.tile)), ("one_tile", tuple(a.small))):
        F, G, res = _timed(lambda: A.find_local_shifts(lag_dx, lag_dy, lag_drot, tile_shape=ts, method=a.method,
                                                       sub_lag=False), A, a.repeat)
        assert np.array_equal(F.corr, G.corr, equal_nan=True)
        assert np.array_equal(F.n_samples.sum(axis=(0, 1)), counts)  # the tiles' counts sum to the untiled ones
        if label == "one_tile":
            assert np.array_equal(F.corr[0, 0], cube, equal_nan=True)  # the bits of the untiled call
        res.update(tile_shape=list(ts), tile_grid=list(F.valid.shape), n_valid=int(F.valid.sum()),
                   pass0_ratio=res["pass0_ms"] / untiled["pass0_ms"], pass1_ratio=res["pass1_ms"] / untiled["pass1_ms"],
                   median_shift=list(F.median_shift), scatter=list(F.scatter))
        runs[label] = res
    pairs = float(small.size) * cube.size
    for res in runs.values():
        res["pairs_per_s"] = [pairs / (res["pass0_ms"] * 1e-3), pairs / (res["pass1_ms"] * 1e-3)]
    out = {"method": a.method, "runs": runs, "counts": [float(counts.min()), float(counts.max())],
           "workload": {"small": list(small.shape), "large": list(large.shape), "lags": list(cube.shape),
                        "ratios": [A.ratio_res_1, A.ratio_res_2], "pixel_pairs_per_pass": pairs}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_tiles_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--tile", type=int, nargs=2, default=(64, 64))
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
               str(a.small[0]), str(a.small[1]), "--tile", str(a.tile[0]), str(a.tile[1]), "--large-n", str(a.large_n),
               "--half", str(a.half), "--n-rot", str(a.n_rot)]
        r = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        if r.returncode != 0:  # (a failure ends the run)
            sys.exit(f"{m}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
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
