#!/usr/bin/env python3
"""
Time of the despiking of SPICE wavelength planes before they are summed (coreg_despike_sum_planes_be) beside the host sum
it replaces (coreg_nansum_planes_be) on the same planes.  A record of what the call costs, nothing is asserted about the
times.

Cases: float32 stacks of 50 x 1024 x 192 and 32 x 832 x 192 pixels as a FITS data unit stores them (big-endian; a line
profile over the planes on unit noise about 500 / plane, 0.5 % NaN pixels, hits on 0.2 % of the pixels of a plane), radius
1, 2 and 3, n_iter 1 and 2, replace = "median", the other parameters at their defaults.  One child process under a time
limit.  Per case, after `--warmup` untimed rounds (the first allocates the buffers), `--repeat` timed ones, the median
reported with every sample kept:
  call_ms          wall time of the whole call on the host: packing the planes, upload, kernels, read-back, wait;
  kernels_ms       the kernels alone by the library's events (coreg_despike_sum_planes_last_ms), with the second LDS window
                   of the last pass (the default) ...
  kernels_serial_ms  ... and without it (handle option "despike_planes_overlap" 0): the same bits, every plane staged before
                   it is decided;
  nansum_ms        wall time of coreg_nansum_planes_be on the same planes (host threads; what runs without the keyword).
The result of the last round is checked against tests/despike_planes_oracle.py on a 24 x 24 corner of three planes, bit for
bit, and the two forms of the last pass against each other on the whole stack.

    python profiles/despike_planes_timing.py [--out profiles/despike_planes_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_stack(shape, seed):
    rng = np.random.default_rng(seed)
    n, ny, nx = shape
    k = np.arange(n) - (n - 1) / 2.0
    prof = 0.2 + np.exp(-0.5 * (k / (n / 8.0)) ** 2)
    v = rng.normal(500.0, 1.0, shape) * prof[:, None, None]
    hit = rng.random(shape) < 0.002
    v[hit] += rng.uniform(100.0, 5000.0, int(hit.sum()))
    v[rng.random(shape) < 0.005] = np.nan
    return v.astype(">f4")


def run_child(a):
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import _lib
    from tests import despike_planes_oracle as PO
    out = {"cases": [], "warmup": a.warmup, "repeat": a.repeat}
    with _lib.CoregHandle(0) as h:
        for shape in ((50, 1024, 192), (32, 832, 192)):
            stack = make_stack(shape, 1)
            idx = np.arange(shape[0])
            nansum = []
            for k in range(a.warmup + a.repeat):
                t0 = time.perf_counter()
                plain = _lib.nansum_planes_be(stack, idx)
                if k >= a.warmup:
                    nansum.append(1e3 * (time.perf_counter() - t0))
            assert plain is not None
            for radius in (1, 2, 3):
                for n_iter in (1, 2):
                    prm = dict(radius=radius, n_iter=n_iter, replace="median")
                    res = {}
                    for overlap in (0, 1):
                        h.set_option("despike_planes_overlap", overlap)
                        call, kern = [], []
                        for k in range(a.warmup + a.repeat):
                            t0 = time.perf_counter()
                            got = h.despike_sum_planes(stack, idx, prm)
                            t1 = time.perf_counter()
                            if k >= a.warmup:
                                call.append(1e3 * (t1 - t0))
                                kern.append(h.despike_sum_planes_last_ms())
                        res[overlap] = (got, call, kern)
                    h.set_option("despike_planes_overlap", 1)
                    got, call, kern = res[1]
                    serial = res[0]
                    assert got[0].tobytes() == serial[0][0].tobytes() and got[1].tobytes() == serial[0][1].tobytes()
                    assert got[2] == serial[0][2]
                    c = 24
                    # (the corner's pixels depend on the corner and n_iter x radius pixels beyond it)
                    reach = c + n_iter * radius
                    corner = np.asarray(stack[:3, :reach, :reach], dtype=np.float32)
                    want = PO.despike_sum_planes(corner, **prm)
                    three = h.despike_sum_planes(stack, [0, 1, 2], prm)
                    assert np.array_equal(three[0][:c, :c], want[0][:c, :c], equal_nan=True)
                    assert np.array_equal(three[1][:c, :c], want[1][:c, :c])
                    out["cases"].append({
                        "shape": list(shape), "dtype": "float32", "radius": radius, "window": 2 * radius + 1, "n_iter": n_iter,
                        "call_ms": float(np.median(call)), "kernels_ms": float(np.median(kern)),
                        "kernels_serial_ms": float(np.median(serial[2])), "call_serial_ms": float(np.median(serial[1])),
                        "nansum_ms": float(np.median(nansum)), "flag_events": got[2],
                        "samples": {"call_ms": call, "kernels_ms": kern, "kernels_serial_ms": serial[2],
                                    "call_serial_ms": serial[1], "nansum_ms": nansum}})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despike_planes_timing.json"))
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=float, default=400.0, help="time limit of the child process [s]")
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
    print(json.dumps({"cases": [{k: v for k, v in c.items() if k != "samples"} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
