#!/usr/bin/env python3
"""
Kernel and call time of the destretch of a local shift field (pxlshift.LocalShiftField.destretch,
coreg_pixels_destretch) on the raster of DESIGN section 9a: 832 x 192 pixels, 50 and 400 wavelength planes, float32 and
float64, a field of (64, 64) tiles -- 13 x 3 nodes -- that drifts by 3 px across the raster, synthetic data.

The kernel moves one read and one write of the cube and is bound by that traffic, so the yardstick is a device-to-device
hipMemcpyAsync of the same cube -- the same bytes read and written -- timed with HIP events in this process, on buffers of
its own.  Per case: one warm-up and `--repeat` timed calls of either; medians with every sample kept; the kernel time is
the library's own (coreg_pixels_destretch_last_ms, HIP events around the kernel), the call time the wall clock of
`LocalShiftField.destretch` (upload, kernel, download).  Four planes of every result are compared with the numpy rule
(tests/pxlshift_destretch_oracle.py) bit for bit.

    python profiles/pxlshift_destretch_timing.py [--out profiles/pxlshift_destretch_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_runtime():
    """The HIP runtime this process has loaded (the one the library runs on)."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    if not paths:
        sys.exit("no HIP runtime is loaded")
    return C.CDLL(sorted(paths)[0])


def _hip(rc, what):
    if rc != 0:
        sys.exit(f"{what}: HIP error {rc}")


def copy_ms(hip, nbytes, repeat):
    """[ms] of `repeat` device-to-device copies of nbytes, after one warm-up copy."""
    src, dst, ev = C.c_void_p(), C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    _hip(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)), "hipMalloc")
    _hip(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)), "hipMalloc")
    _hip(hip.hipMemset(src, 1, C.c_size_t(nbytes)), "hipMemset")
    for e in ev:
        _hip(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = []
    for k in range(repeat + 1):
        _hip(hip.hipEventRecord(ev[0], None), "hipEventRecord")
        _hip(hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None), "hipMemcpyAsync")  # 3: device to device
        _hip(hip.hipEventRecord(ev[1], None), "hipEventRecord")
        _hip(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = C.c_float(0.0)
        _hip(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        if k:
            out.append(float(ms.value))
    for e in ev:
        hip.hipEventDestroy(e)
    hip.hipFree(src)
    hip.hipFree(dst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxlshift_destretch_timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=2, default=(832, 192))
    ap.add_argument("--tile", type=int, nargs=2, default=(64, 64))
    ap.add_argument("--planes", type=int, nargs="+", default=(50, 400))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.pxlshift import LocalShiftField
    from tests import pxlshift_destretch_oracle as D

    (h, w), tile = a.small, tuple(a.tile)
    grid = (-(-h // tile[0]), -(-w // tile[1]))
    # a field whose best lags drift by 3 px along the raster's columns and by 2 px along its rows (no sub-lag fit)
    lag = np.arange(-3, 4)
    corr = np.full(grid + (7, 7, 1), 0.1)
    for ty in range(grid[0]):
        for tx in range(grid[1]):
            corr[ty, tx, 3 + round(-1.5 + 3.0 * tx / max(grid[1] - 1, 1)), 3 + round(1.0 - 2.0 * ty / max(grid[0] - 1, 1)), 0] = 0.9
    F = LocalShiftField(corr, np.full(corr.shape, float(tile[0] * tile[1])), lag, lag, [0.0], tile, (h, w), sub_lag=False)
    hnd = _lib.shared_handle(-1)
    hip = _hip_runtime()
    rng = np.random.default_rng(9)
    cases = {}
    for n_planes in a.planes:
        base = rng.uniform(1.0, 9.0, (n_planes, h, w))
        for dtype in ("float32", "float64"):
            cube = base.astype(dtype)
            first = F.destretch(cube)  # warm-up
            kernel, calls = [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                again = F.destretch(cube)
                calls.append(time.perf_counter() - t0)
                kernel.append(hnd.pixels_destretch_last_ms())
            assert np.array_equal(first, again, equal_nan=True)
            for k in sorted({0, min(7, n_planes - 1), min(8, n_planes - 1), n_planes - 1}):
                want = D.field_destretch(F, cube[k])
                assert np.array_equal(np.isnan(again[k]), np.isnan(want)) and np.array_equal(again[k][~np.isnan(want)],
                                                                                              want[~np.isnan(want)])
            copies = copy_ms(hip, cube.nbytes, a.repeat)
            k_ms, c_ms = float(np.median(kernel)), float(np.median(copies))
            moved = 2 * cube.nbytes  # one read and one write of the cube
            cases[f"{n_planes}_planes_{dtype}"] = {
                "n_planes": n_planes, "dtype": dtype, "bytes_moved": moved, "kernel_ms": k_ms, "kernel_ms_samples": kernel,
                "copy_ms": c_ms, "copy_ms_samples": copies, "kernel_over_copy": k_ms / c_ms,
                "kernel_GB_per_s": moved / (k_ms * 1e-3) / 1e9, "copy_GB_per_s": moved / (c_ms * 1e-3) / 1e9,
                "call_s": float(np.median(calls)), "calls_s": calls, "nan_fraction": float(np.isnan(again).mean())}
            print(f"{n_planes} planes {dtype}: kernel {k_ms:.4f} ms, copy {c_ms:.4f} ms, ratio {k_ms / c_ms:.2f}, call "
                  f"{np.median(calls):.4f} s", flush=True)
    res = {"workload": {"raster": [h, w], "tile_shape": list(tile), "nodes": list(grid), "interpolation": "bilinear",
                        "median_shift": list(F.median_shift), "plane_chunk": 8, "repeat": a.repeat}, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
