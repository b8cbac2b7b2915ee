#!/usr/bin/env python3
"""
Pass times of the mutual-information score of the pixel-lag sweep (pxlshift, method "mutual_information") at 8, 16 and 32
bins beside the two Pearson passes and the two residus_masked passes of the same process, untiled and in tiles of
(64, 64), on the workload of profiles/pxlshift_scores_timing.py: an 832 x 192 raster against a 3072 x 3072 image, ratios
(0.94, 0.247), 61 x 61 x 21 lags (1.25e10 pixel pairs per pass), synthetic data.

One child process under a time limit runs every configuration through the library calls of `AlignmentPixels` (images set
once; coreg_pixels_sweep_method / coreg_pixels_sweep_tiles): one warm-up call, then `--repeat` timed calls; the library's
HIP-event times (coreg_pixels_last_timing) are reported as medians with every sample kept, and as pixel pairs per second.
The histogram pass is `pass0_ms`; `pass1_ms` of that score lies between two events with nothing between them.

    python profiles/pxlshift_mi_timing.py [--out profiles/pxlshift_mi_timing.json]
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


def _timed(call, hnd, repeat, pairs):
    first = call()  # warm-up
    calls, t = [], {k: [] for k in SPANS}
    for _ in range(repeat):
        t0 = time.perf_counter()
        again = call()
        calls.append(time.perf_counter() - t0)
        lt = hnd.pixels_last_timing()
        for k in SPANS:
            t[k].append(lt[k])
    assert np.array_equal(first, again, equal_nan=True)
    res = {"call_s": float(np.median(calls)), "calls_s": calls}
    for k, v in t.items():
        res[k] = float(np.median(v))
        res[k + "_samples"] = v
    res["pass0_pairs_per_s"] = pairs / (res["pass0_ms"] * 1e-3)
    return first, res


def run_child(a):
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import _lib, synthetic
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    lcd = 4.44 * 3072 / a.large_n
    small, hs, large, hl, _ = synthetic.make_scene(small_shape=tuple(a.small), large_n=a.large_n, n_blobs=300,
                                                   small_cdelt=(0.94 * lcd, 0.247 * lcd), large_crval=(-310.0, 420.0))
    A = AlignmentPixels((large, hl), 0, (small, hs), 0)
    lag_dx = lag_dy = np.arange(-a.half, a.half + 1)
    lag_drot = np.linspace(-1.0, 1.0, a.n_rot)
    hnd = _lib.shared_handle(-1)
    hnd.pixels_set_large(A.data_large)
    hnd.pixels_set_small(A.data_small)
    pairs = float(small.size) * len(lag_dx) * len(lag_dy) * len(lag_drot)
    configs = [("correlation", None), ("residus_masked", None)] + [("mutual_information", b) for b in a.bins]
    runs = {}
    for method, bins in configs:
        kw = {} if bins is None else {"bins": bins}
        plan = A.host_plan(lag_dx, lag_dy, lag_drot, method=method, tile_shape=tuple(a.tile), **kw)
        label = method if bins is None else f"{method}_B{bins}"
        cube, untiled = _timed(lambda: hnd.pixels_sweep(plan, plan["method_code"]), hnd, a.repeat, pairs)
        counts = hnd.pixels_last_counts(cube.shape)
        tiles, tiled = _timed(lambda: hnd.pixels_sweep_tiles(plan, plan["method_code"]), hnd, a.repeat, pairs)
        assert np.array_equal(hnd.pixels_last_tile_counts(tiles.shape).sum(axis=(0, 1)), counts)
        if method != "mutual_information":
            for r in (untiled, tiled):
                r["pass1_pairs_per_s"] = pairs / (r["pass1_ms"] * 1e-3)
        else:
            untiled["edges"] = [len(e) for e in plan["bins"]]
        best = (np.nanargmin if method == "residus_masked" else np.nanargmax)(cube)
        untiled.update(best_index=[int(v) for v in np.unravel_index(best, cube.shape)], n_nan=int(np.isnan(cube).sum()),
                       best=float(cube.ravel()[best]), counts=[float(counts.min()), float(counts.max())])
        tiled.update(tile_shape=list(a.tile), tile_grid=list(tiles.shape[:2]),
                     pass0_ratio=tiled["pass0_ms"] / untiled["pass0_ms"])
        runs[label] = {"untiled": untiled, "tiles": tiled}
    out = {"runs": runs, "workload": {"small": list(small.shape), "large": list(large.shape),
                                      "lags": [len(lag_dx), len(lag_dy), len(lag_drot)],
                                      "ratios": [plan["ratio_res_1"], plan["ratio_res_2"]], "pixel_pairs_per_pass": pairs}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_mi_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--tile", type=int, nargs=2, default=(64, 64))
    ap.add_argument("--bins", type=int, nargs="+", default=(8, 16, 32))
    ap.add_argument("--large-n", type=int, default=3072)
    ap.add_argument("--half", type=int, default=30, help="dx, dy in [-half, half]")
    ap.add_argument("--n-rot", type=int, default=21)
    ap.add_argument("--limit", type=float, default=400.0, help="time limit of the child process [s]")
    ap.add_argument("--child", action="store_true", help="(child) run the configurations in this process")
    a = ap.parse_args()
    if a.child:
        return run_child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--small", str(a.small[0]),
           str(a.small[1]), "--tile", str(a.tile[0]), str(a.tile[1]), "--large-n", str(a.large_n), "--half", str(a.half),
           "--n-rot", str(a.n_rot), "--bins"] + [str(b) for b in a.bins]
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
