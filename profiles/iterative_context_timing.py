"""Cost of the iterative-context SPICE sweep (AlignementSpiceIterativeContextRaster, include/coreg_hip.h:
coreg_sweep_context) on a realistic raster: a 192-step x 800-row SPICE window, 16 imager frames of 2048^2 (float32),
a 61 x 61 CRVAL grid.  Timed three ways on one GPU:
  fused            one coreg_sweep_context call (plan on the host + the fused kernel + finalize), wall time
  spice_sweep      the existing SPICE sweep (coreg_sweep_helioprojective, one fixed reference on the same grid), for
                   the per-lag-point cost the fused sweep is compared with
  per_lag          the per-lag composition through the existing calls (resample_helioprojective of every used frame +
                   of the SPICE image, Pearson in NumPy), timed on a few lag-points and extrapolated to the grid
Writes one JSON object to stdout (and to the path given as the first argument)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from euispice_coreg_amd import _lib  # noqa: E402


def scene(nx=192, ny=800, n_frames=16, fsize=2048, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:fsize, 0:fsize].astype(np.float32)
    base = (1000.0 + 300.0 * np.sin(xx / 37.0) * np.cos(yy / 53.0)).astype(np.float32)
    frames = [(base + rng.normal(0, 5.0, base.shape).astype(np.float32)).astype(np.float32) for _ in range(n_frames)]
    fh = []
    for k in range(n_frames):
        fh.append({"NAXIS1": fsize, "NAXIS2": fsize, "CRPIX1": (fsize + 1) / 2, "CRPIX2": (fsize + 1) / 2,
                   "CRVAL1": 0.3 * k, "CRVAL2": -0.2 * k, "CDELT1": 4.44, "CDELT2": 4.44, "CUNIT1": "arcsec",
                   "CUNIT2": "arcsec", "CTYPE1": "HPLN-TAN", "CTYPE2": "HPLT-TAN", "PC1_1": 1.0, "PC1_2": 0.0,
                   "PC2_1": 0.0, "PC2_2": 1.0, "CROTA": 0.0})
    rho = np.deg2rad(3.0)
    lam = 1.098 / 4.0
    small = {"NAXIS1": nx, "NAXIS2": ny, "CRPIX1": (nx + 1) / 2, "CRPIX2": (ny + 1) / 2,
             "CRVAL1": float("%.14G" % (-300.0 / 3600)), "CRVAL2": float("%.14G" % (400.0 / 3600)),
             "CDELT1": float("%.14G" % (4.0 / 3600)), "CDELT2": float("%.14G" % (1.098 / 3600)), "CUNIT1": "deg",
             "CUNIT2": "deg", "CTYPE1": "HPLN-TAN", "CTYPE2": "HPLT-TAN", "PC1_1": float("%.14G" % np.cos(rho)),
             "PC1_2": float("%.14G" % (-lam * np.sin(rho))), "PC2_1": float("%.14G" % (np.sin(rho) / lam)),
             "PC2_2": float("%.14G" % np.cos(rho)), "CROTA": 3.0}
    target = dict(small, CRVAL1=-300.0 / 3600, CRVAL2=400.0 / 3600, CDELT1=4.0 / 3600, CDELT2=1.098 / 3600,
                  PC1_1=np.cos(rho), PC1_2=-lam * np.sin(rho), PC2_1=np.sin(rho) / lam, PC2_2=np.cos(rho))
    data = np.asarray(rng.normal(500.0, 80.0, (ny, nx)), dtype=np.float64)
    data[:40] = np.nan
    data[-40:] = np.nan
    col_frame = (np.arange(nx) * n_frames // nx).astype(np.int32)
    return frames, fh, small, target, data, col_frame


def main():
    frames, fh, small, target, data, col_frame = scene()
    step = 1.0 / 3600
    lags = _lib.LagSet(np.arange(-30, 31) * step, np.arange(-30, 31) * step, None, None, None)
    res = {"raster": [800, 192], "frames": [16, 2048, 2048], "frame_dtype": "float32", "lags": list(lags.shape[:2])}
    with _lib.CoregHandle(0) as h:
        t = time.perf_counter()
        h.set_context_frames(frames, fh)
        h.synchronize()
        res["set_context_frames_s"] = time.perf_counter() - t
        h.set_small(data)
        h.sweep_context(target, small, col_frame, lags)  # warm-up
        walls, kern = [], []
        for _ in range(5):
            t = time.perf_counter()
            corr = h.sweep_context(target, small, col_frame, lags)
            walls.append(time.perf_counter() - t)
            kern.append(h.last_stats()["sweep_kernel_ms"])
        res["fused_wall_ms"] = [1e3 * w for w in walls]
        res["fused_kernel_ms"] = kern
        res["fused_ns_per_lag_point"] = 1e9 * min(walls) / lags.size
        res["fused_finite"] = int(np.isfinite(corr).sum())
        # the existing SPICE sweep on the same grid and lags (one fixed reference: the zero-lag context)
        h.set_small(frames[0])
        ctx0 = h.resample_helioprojective(target, fh[0], order=2, dtype=np.float64)
        h.set_small(data)
        h.set_reference_on_grid(ctx0)
        h.sweep_helioprojective(small, small, lags)
        walls = []
        for _ in range(5):
            t = time.perf_counter()
            h.sweep_helioprojective(small, small, lags)
            walls.append(time.perf_counter() - t)
        res["spice_sweep_wall_ms"] = [1e3 * w for w in walls]
        res["spice_sweep_kernel_ms"] = h.last_stats()["sweep_kernel_ms"]
        res["spice_sweep_ns_per_lag_point"] = 1e9 * min(walls) / lags.size
        # per-lag composition through the existing calls, a few lag-points
        used = sorted(set(col_frame.tolist()))
        n_probe = 8
        t = time.perf_counter()
        for q in range(n_probe):
            r = _lib.context_lag_headers(target, small, lags.arrays[0][q * 7], lags.arrays[1][q * 5], 0.0, 0.0, 0.0)
            hc, hg, hs = (_lib.wcs_to_dict(w) for w in r)
            large = np.empty((800, 192))
            for f in used:
                h.set_small(frames[f])
                cols = np.nonzero(col_frame == f)[0]
                large[:, cols] = h.resample_helioprojective(hc, fh[f], order=2, dtype=np.float32)[:, cols]
            h.set_small(data)
            b = h.resample_helioprojective(hg, hs, order=2, dtype=np.float32).astype(np.float64).ravel()
            a = large.ravel()
            m = ~np.isnan(a) & ~np.isnan(b)
            np.corrcoef(a[m], b[m])
        per = (time.perf_counter() - t) / n_probe
        res["per_lag_s_per_lag_point"] = per
        res["per_lag_extrapolated_s"] = per * lags.size
        res["speedup_fused_vs_per_lag"] = per * lags.size / (min(res["fused_wall_ms"]) / 1e3)
        res["fused_over_spice_sweep_per_lag_point"] = res["fused_ns_per_lag_point"] / res["spice_sweep_ns_per_lag_point"]
    out = json.dumps(res, indent=1)
    print(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
