#!/usr/bin/env python3
"""
Time of the median/MAD despiking of the resident image to align (coreg_despike_small: one pass of k_despike_image and the
pivot) beside the correlation sweep of the same process.  A record of what the kernel costs, nothing is asserted about the
times.

Cases: a 2048 x 2048 float32 image and a 4096 x 4096 float64 image (unit noise about 500, 0.5 % NaN pixels, 0.5 % spikes),
radius 1, 2 and 3, one pass, the other parameters at their defaults.  One child process under a time limit.  The handle
runs on a stream of torch's, so that HIP events recorded on that stream bracket exactly the work of one call: per case the
image is uploaded and the stream drained, then event, coreg_despike_small (counts not read back: no host wait inside),
event -- `--warmup` untimed rounds (the first allocates the buffers), then `--repeat` timed ones; the median is reported
with every sample kept.  The result of the last round is checked against tests/despike_oracle.py on a 64 x 64 corner, bit
for bit.  The sweep beside it is the README's headline workload (2048 x 2048 lon/lat grid, 60 x 60 CRVAL lags, order 2),
timed by the library's own events (coreg_last_stats).

    python profiles/despike_timing.py [--out profiles/despike_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONLIMS, LATLIMS, SOLAR_R = (200.0, 300.0), (-20.0, 20.0), 1.004


def run_child(a):
    sys.path.insert(0, ROOT)
    import torch
    from euispice_coreg_amd import _lib, synthetic
    from tests import despike_oracle as DO
    stream = torch.cuda.Stream()
    out = {"cases": [], "warmup": a.warmup, "repeat": a.repeat, "selection": "sorting network"}
    with _lib.CoregHandle(0) as h:
        h.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(1)
        for n, dtype in ((2048, np.float32), (4096, np.float64)):
            img = rng.normal(500.0, 1.0, (n, n))
            hit = rng.random(img.shape) < 0.005
            img[hit] += rng.uniform(300.0, 5000.0, int(hit.sum()))
            img = img.astype(np.float32) if dtype == np.float32 else img + 1e-9
            img[rng.random(img.shape) < 0.005] = np.nan
            for radius in (1, 2, 3):
                prm = dict(radius=radius, n_iter=1)
                p = _lib.DespikeParams.of(prm)
                samples = []
                for k in range(a.warmup + a.repeat):
                    h.set_small(img)
                    h.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        rc = h._lib.coreg_despike_small(h._h, C.byref(p), None)
                        e1.record()
                    assert rc == 0, rc
                    e1.synchronize()
                    if k >= a.warmup:
                        samples.append(float(e0.elapsed_time(e1)))
                got = h.get_small(img.shape, img.dtype)
                c = 64
                # (the corner's pixels depend on the corner and `radius` pixels beyond it)
                want, _ = DO.despike(img[:c + radius, :c + radius], **prm)
                assert np.array_equal(got[:c, :c], want[:c, :c], equal_nan=True)
                ms = float(np.median(samples))
                out["cases"].append({"shape": [n, n], "dtype": np.dtype(dtype).name, "radius": radius,
                                     "window": 2 * radius + 1, "n_iter": 1, "despike_small_ms": ms, "samples_ms": samples,
                                     "pixels_per_us": n * n / ms / 1e3,
                                     "flagged": int(np.isfinite(img).sum() - np.isfinite(got).sum())})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despike_timing.json"))
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
