#!/usr/bin/env python3
"""
Time of the NaN-aware smoothing of the resident image to align (coreg_smooth_small: row pass, column pass, pivot) beside
the correlation sweep of the same process.  A record of what the kernels cost, nothing is asserted about the times.

Cases: a 2048 x 2048 float32 image and a 4096 x 4096 float64 image (0.5 % NaN pixels), Gaussian tables of reach r = 8 and
r = 64 on both axes.  One child process under a time limit.  The handle runs on a stream of torch's, so that HIP events
recorded on that stream bracket exactly the work of one call: per case the image is uploaded and the stream drained, then
event, coreg_smooth_small, event -- `--warmup` untimed rounds (the first allocates the planes), then `--repeat` timed ones;
the median is reported with every sample kept, and the bytes the two passes move at the least (source read twice, two
planes written and read, result written) over that time.  The result of the last round is checked against
tests/smooth_oracle.py on a 96 x 96 corner.  The sweep beside it is the README's headline workload (2048 x 2048 lon/lat grid,
60 x 60 CRVAL lags, order 2), timed by the library's own events (coreg_last_stats).

    python profiles/smooth_timing.py [--out profiles/smooth_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONLIMS, LATLIMS, SOLAR_R = (200.0, 300.0), (-20.0, 20.0), 1.004


def table(r):
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * (r / 4.0) ** 2))
    return w / w.sum()


def run_child(a):
    sys.path.insert(0, ROOT)
    import torch
    from euispice_coreg_amd import _lib, synthetic
    from tests import smooth_oracle as SO
    stream = torch.cuda.Stream()
    out = {"cases": [], "warmup": a.warmup, "repeat": a.repeat}
    with _lib.CoregHandle(0) as h:
        h.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(1)
        for n, dtype in ((2048, np.float32), (4096, np.float64)):
            img = rng.normal(500.0, 100.0, (n, n))
            img = img.astype(np.float32) if dtype == np.float32 else img + 1e-9
            img[rng.random(img.shape) < 0.005] = np.nan
            for r in (8, 64):
                w = table(r)
                samples = []
                for k in range(a.warmup + a.repeat):
                    h.set_small(img)
                    h.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        h.smooth_small((w, w))
                        e1.record()
                    e1.synchronize()
                    if k >= a.warmup:
                        samples.append(float(e0.elapsed_time(e1)))
                got = h.get_small(img.shape)
                c = min(96, n)
                # (the corner's pixels depend on the corner and r pixels beyond it)
                want = SO.smooth(img[:c + r, :c + r], w, w)[:c, :c]
                bound = SO.bound(img[:c + r, :c + r], w, w)[:c, :c]
                assert np.array_equal(np.isnan(got[:c, :c]), np.isnan(want)) and np.nanmax(np.abs(got[:c, :c] - want) - bound) <= 0
                ms = float(np.median(samples))
                elem = np.dtype(dtype).itemsize
                moved = n * n * (2 * elem + 2 * 8 + 2 * 8 + 8)
                out["cases"].append({"shape": [n, n], "dtype": np.dtype(dtype).name, "r": r, "taps": 2 * r + 1,
                                     "smooth_small_ms": ms, "samples_ms": samples, "min_bytes_moved": moved,
                                     "min_bytes_over_time_GBps": moved / ms / 1e6})
        # the correlation sweep of the same process
        small, hs, large, hl, _ = synthetic.make_scene(small_n=2048, large_n=3072)
        grid = _lib.Grid(LONLIMS, LATLIMS, (2048, 2048))
        lag = np.arange(-30.0, 30.0, 1.0)
        lags = _lib.LagSet(lag, lag, None, None, None)
        h.set_small(small.astype(np.float32))
        h.prepare_reference_carrington(large.astype(np.float32), hl, grid, SOLAR_R, 2)
        spans = []
        for k in range(a.warmup + a.repeat):
            h.sweep_carrington(hs, grid, SOLAR_R, lags, order=2)
            if k >= a.warmup:
                spans.append(float(h.last_stats()["total_gpu_ms"]))
        out["correlation_sweep"] = {"grid": [2048, 2048], "lags": [len(lag), len(lag)], "order": 2, "small": [2048, 2048],
                                    "total_gpu_ms": float(np.median(spans)), "samples_ms": spans}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_timing.json"))
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0, help="time limit of the child process [s]")
    ap.add_argument("--child", action="store_true", help="(child) run the measurements in this process")
    a = ap.parse_args()
    if a.child:
        return run_child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--warmup", str(a.warmup)]
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
