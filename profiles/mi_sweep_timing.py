#!/usr/bin/env python3
"""
Time of the mutual-information sweep of the Carrington frame (coreg_sweep_carrington, COREG_METHOD_MUTUAL_INFORMATION, 16
quantile bins per image) beside the Pearson sweep of the same process, on the README's headline workload: 2048 x 2048
lon/lat grid, lon (200, 300), lat (-20, 20), 60 x 60 CRVAL lags, synthetic 2048^2 image against a 3072^2 reference, both
images resident on the device.  No threshold: a record of what the kernel costs.

One child process under a time limit: the reference is prepared once; per method `--warmup` untimed sweeps, then `--repeat`
timed ones, each a synchronous library call (host output: the call returns when the map is on the host) timed with the host
clock around it, and with the library's own HIP events around its kernels (coreg_last_stats: sweep kernel, precompute,
first launch to last).  The two methods alternate sweep by sweep, so that a drift of the machine hits both.  Medians are
reported with every sample kept; the ratio is the quotient of the median call times.  The two maps are checked against
each other where that is possible: equal sample counts entry for entry, every entry finite, and the argmax.

    python profiles/mi_sweep_timing.py [--out profiles/mi_sweep_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONLIMS, LATLIMS, SOLAR_R = (200.0, 300.0), (-20.0, 20.0), 1.004
SPANS = ("sweep_kernel_ms", "precompute_ms", "total_gpu_ms")


def run_child(a):
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import _lib, synthetic
    from euispice_coreg_amd.hdrshift.alignment import default_edges
    small, hs, large, hl, truth = synthetic.make_scene(small_n=a.small_n, large_n=a.large_n)
    shape = (a.grid, a.grid)
    lag = np.arange(-a.half, a.half, 1.0)
    lags = _lib.LagSet(lag, lag, None, None, None)
    grid = _lib.Grid(LONLIMS, LATLIMS, shape)
    h = _lib.shared_handle(-1)
    h.set_small(small)
    h.prepare_reference_carrington(large, hl, grid, SOLAR_R, 2)
    es, el = default_edges(small, None, None, h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64), a.bins)
    h.sweep_set_bins(es, el)
    methods = {"correlation": _lib.METHOD_CORRELATION, "mutual_information": _lib.METHOD_MUTUAL_INFORMATION}

    def sweep(name):
        t0 = time.perf_counter()
        out = h.sweep_carrington(hs, grid, SOLAR_R, lags, order=2, method=methods[name])
        dt = time.perf_counter() - t0
        return out, dt, h.last_stats()

    maps, counts = {}, {}
    for name in methods:
        for _ in range(a.warmup):
            maps[name] = sweep(name)[0]
        counts[name] = h.last_counts()
    runs = {name: {"calls_s": [], **{k + "_samples": [] for k in SPANS}} for name in methods}
    for _ in range(a.repeat):
        for name in methods:  # (alternating)
            out, dt, st = sweep(name)
            assert np.array_equal(out, maps[name], equal_nan=True), name + ": a repeated sweep gave other bits"
            runs[name]["calls_s"].append(dt)
            for k in SPANS:
                runs[name][k + "_samples"].append(st[k])
            runs[name]["n_sweep_launches"] = int(st["n_sweep_launches"])
            runs[name]["n_active_points"] = int(st["n_active_points"])
    for name, r in runs.items():
        r["call_s"] = float(np.median(r["calls_s"]))
        for k in SPANS:
            r[k] = float(np.median(r[k + "_samples"]))
        m = maps[name]
        r["n_nan"] = int(np.isnan(m).sum())
        r["best_index"] = [int(v) for v in np.unravel_index(np.nanargmax(m), lags.shape)[:2]]
        r["best"] = float(np.nanmax(m))
        r["counts"] = [float(np.nanmin(counts[name])), float(np.nanmax(counts[name]))]
    assert np.array_equal(counts["correlation"], counts["mutual_information"]), "the two methods count other pairs"
    mi, pe = runs["mutual_information"], runs["correlation"]
    out = {"runs": runs,
           "ratio_call_time_mi_over_correlation": mi["call_s"] / pe["call_s"],
           "ratio_sweep_kernel_mi_over_correlation": mi["sweep_kernel_ms"] / pe["sweep_kernel_ms"],
           "same_argmax": mi["best_index"] == pe["best_index"],
           "injected_lag": [truth["lag_crval1"], truth["lag_crval2"]],
           "workload": {"grid": list(shape), "lonlims": list(LONLIMS), "latlims": list(LATLIMS), "small": list(small.shape),
                        "large": list(large.shape), "lags": [len(lag), len(lag)], "order": 2, "bins": a.bins,
                        "edges": [len(es), len(el)], "warmup": a.warmup, "repeat": a.repeat,
                        "sample_pairs_per_sweep": float(np.nansum(counts["correlation"]))}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi_sweep_timing.json"))
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--small-n", type=int, default=2048)
    ap.add_argument("--large-n", type=int, default=3072)
    ap.add_argument("--half", type=int, default=30, help="CRVAL lags arange(-half, half, 1) arcsec on both axes")
    ap.add_argument("--limit", type=float, default=400.0, help="time limit of the child process [s]")
    ap.add_argument("--child", action="store_true", help="(child) run the sweeps in this process")
    a = ap.parse_args()
    if a.child:
        return run_child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--warmup", str(a.warmup),
           "--bins", str(a.bins), "--grid", str(a.grid), "--small-n", str(a.small_n), "--large-n", str(a.large_n),
           "--half", str(a.half)]
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
