#!/opt/conda/bin/python3.9
"""
Golden-vector generator (reference) for the iterative-context SPICE alignment: the REFERENCE's own
`AlignementSpiceIterativeContextRaster._step` (`hdrshift/alignment_spice.py:361-421`), after its own
`_extract_spice_data_header` / `_prepare_spice_from_l2` (:467-469) and `_extract_imager_data_header` (:423-432), on
two of the four random SPICE windows and imager sequences of `synras_fuzz_golden` (P00: 15 frames used, P05: 5), one
`_step` per lag-point.

The reference class cannot run as committed; four stated shims, nothing else:
  1. constructor keywords: `__init__` passes `use_tqdm`, `small_fov_value_min`, `small_fov_value_max` to an
     `AlignmentSpice.__init__` that takes none of them (TypeError) -> `AlignmentSpice.__init__` with the keywords it
     does take, then the class's own attribute assignments (:366-369) and the two thresholds;
  2. `index_amplitude -> coeff`: `align_using_helioprojective` calls `_extract_spice_data_header(level,
     index_amplitude=...)` (TypeError) -> the same call with `coeff=`;
  3. `ComposedMapBuilder.process_from_header(path_output=None)` ends in `os.path.join(None, ...)` (TypeError, after
     the map and header are made, `map_builder.py:211`) -> that TypeError is caught;
  4. `_step` shifts the unflattened 4-D header, whose CUNIT1/2 are arcsec, with lags and *_ref values already in the
     flattened header's degrees, and `_shift_header` raises "lag.unit and cUNIT are not the same"
     (`alignment.py:403-406`) -> the unflattened header's CRVAL1/2 and CDELT1/2 are converted to degrees
     (x u.arcsec.to(u.deg)), CUNIT1/2 = 'deg', right after `_prepare_spice_from_l2`.
Also: `_find_best_header_parameters`' serial branch never calls `_step` (it calls `_step_no_shmm`, `alignment.py:765-797`),
so `_step` is driven here directly over the C-order lag grid (the order of `alignment.py:667-674`).

A lag never changes which frame a column takes: `_shift_header` writes CRVAL / CDELT / CROTA / PC1_1..PC2_2 only, and
the slit times come from the time row of the PC matrix (PC4_1) and CDELT4 / CRVAL4 (`map_builder.py:253-280`).

    tests/golden/iterative_context_golden.npz    corr map of every case, frame of every column
    tests/golden/iterative_context_golden.json   cases: window, lags (arcsec / deg), thresholds, method

Inputs are rebuilt by the tests from `spice_fuzz_golden` / `synras_fuzz_golden` (deterministic).

Run (build container only, after make_golden_synras_fuzz.py; about a minute):
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_iterative_context.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_callers as M  # noqa: E402  (loads the reference through _reference_loader)
from make_golden_spice_fuzz import build_cube  # noqa: E402

import numpy as np  # noqa: E402
import astropy.units as u  # noqa: E402
from astropy.io import fits  # noqa: E402
from euispice_coreg.hdrshift import alignment_spice as AS  # noqa: E402
from euispice_coreg.synras import map_builder as MB  # noqa: E402

CLS = AS.AlignementSpiceIterativeContextRaster

# shim 2
CLS._extract_spice_data_header = (lambda self, level, index_amplitude=None:
                                  AS.AlignmentSpice._extract_spice_data_header(self, level=level, coeff=index_amplitude))

# shim 3
_pfh = MB.ComposedMapBuilder.process_from_header


def _process_from_header(self, *a, **k):
    try:
        _pfh(self, *a, **k)
    except TypeError:
        if getattr(self, "hdr_composed", None) is None:
            raise


MB.ComposedMapBuilder.process_from_header = _process_from_header

# shim 4
_prep = CLS._prepare_spice_from_l2


def _prepare_spice_from_l2(self, hdul_small):
    _prep(self, hdul_small)
    h = self.header_spice_unflattened
    for k in (1, 2):
        if str(h[f"CUNIT{k}"]).strip() != "deg":
            f = u.Unit(str(h[f"CUNIT{k}"]).strip()).to(u.deg)
            h[f"CRVAL{k}"] = h[f"CRVAL{k}"] * f
            h[f"CDELT{k}"] = h[f"CDELT{k}"] * f
            h[f"CUNIT{k}"] = "deg"


CLS._prepare_spice_from_l2 = _prepare_spice_from_l2


def make(paths, p_spice, threshold, lags, vmin=None, vmax=None):
    """shim 1: the constructor"""
    A = CLS.__new__(CLS)
    AS.AlignmentSpice.__init__(A, large_fov_known_pointing="No_specific_path", small_fov_to_correct=p_spice,
                               lag_crval1=lags[0], lag_crval2=lags[1], lag_cdelt1=lags[2], lag_cdelt2=lags[3],
                               lag_crota=lags[4], lag_solar_r=None, parallelism=False, counts_cpu_max=40,
                               large_fov_window=-1, small_fov_window=0, path_save_figure=None)
    A.small_fov_value_min, A.small_fov_value_max = vmin, vmax
    A.step_figure = False
    A.large_fov_list_paths = paths
    A.small_fov_to_correct = p_spice
    A.threshold_time = u.Quantity(threshold, "s")
    return A


def run_steps(A, method):
    """align_using_helioprojective (:437-465) up to the sweep, then `_step` over the lag grid."""
    A.lonlims = A.latlims = A.shape = A.reference_date = None
    A.function_to_apply = A._interpolate_on_large_data_grid
    A.method = method
    A.coordinate_frame = "final_helioprojective"
    A.extend_pixel_size = False
    A.lon_ctype, A.lat_ctype = "HPLN-TAN", "HPLT-TAN"
    with contextlib.redirect_stdout(io.StringIO()):
        A._extract_spice_data_header(level=2, index_amplitude=None)
        A._extract_imager_data_header()
        A._set_initial_header_values(True)
    L = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in
         (A.lag_crval1, A.lag_crval2, A.lag_cdelt1, A.lag_cdelt2, A.lag_crota)]
    out = np.full([len(v) for v in L], np.nan)
    for idx in np.ndindex(out.shape):
        d = [L[k][idx[k]] for k in range(5)]
        with contextlib.redirect_stdout(io.StringIO()):
            r = A._step(d_crval2=d[1], d_crval1=d[0], d_cdelt1=d[2], d_cdelt2=d[3], d_crota=d[4], d_solar_r=1.004,
                        method=method)
        out[idx] = float(np.asarray(r).ravel()[0])
    return out, [v.tolist() for v in L]


CASES = {
    # name: window, lags in arcsec (crota in deg), thresholds, method
    "P00_crval": ("P00", ((np.arange(7) - 3) * 2.0, (np.arange(7) - 3) * 1.5, None, None, None), None, None, "correlation"),
    "P05_crval_min": ("P05", ((np.arange(7) - 3) * 3.0, (np.arange(7) - 3) * 2.0, None, None, None), 60.0, None,
                      "correlation"),
    "P00_crota": ("P00", ((np.arange(3) - 1) * 2.0, (np.arange(3) - 1) * 2.0, None, None, [-0.5, 0.0, 0.5]), None, None,
                  "correlation"),
    "P05_cdelt1": ("P05", ((np.arange(3) - 1) * 3.0, (np.arange(3) - 1) * 3.0, [-0.2, 0.0, 0.2], None, None), None,
                   None, "correlation"),
    "P00_residus_min": ("P00", ((np.arange(5) - 2) * 2.0, (np.arange(5) - 2) * 2.0, None, None, None), 60.0, None,
                        "residus"),
}


def main():
    tmp = tempfile.mkdtemp(prefix="golden_iterative_context_")
    g = np.load(os.path.join(HERE, "spice_fuzz_golden.npz"))
    with open(os.path.join(HERE, "spice_fuzz_golden.json")) as f:
        sp = json.load(f)["scenes"]
    with open(os.path.join(HERE, "synras_fuzz_golden.json")) as f:
        sf = json.load(f)["cases"]
    scenes = {}
    for name in sorted(set(c[0] for c in CASES.values())):
        h4, hl = dict(sp[name]["hdr4d"]), dict(sp[name]["hdr_large"])
        cube = build_cube(g[f"{name}/image"], g[f"{name}/profile"], g[f"{name}/nan_voxels"], g[f"{name}/nan_spectra"])
        d = os.path.join(tmp, name)
        os.makedirs(d)
        p_spice = os.path.join(d, sp[name]["file"])
        fits.HDUList([fits.PrimaryHDU(data=cube, header=M.to_header(h4))]).writeto(p_spice, overwrite=True)
        c = sf[name]
        frames = M.synthetic.make_imager_sequence(g[f"{name}/large"].astype(np.float64), hl, start=c["start"],
                                                  cadence_s=c["cadence_s"], n_frames=c["n_frames"])
        paths = []
        for j, (img, h) in enumerate(frames):
            p = os.path.join(d, f"solo_L2_eui-fsi174-image_{j:02d}.fits")
            fits.HDUList([fits.PrimaryHDU(), fits.ImageHDU(data=img, header=M.to_header(h))]).writeto(p, overwrite=True)
            paths.append(p)
        scenes[name] = (paths, p_spice, c["threshold_time"])
    ARR, META = {}, {"cases": {}, "interpreter": {}}
    for cname, (name, lags, vmin, vmax, method) in CASES.items():
        paths, p_spice, thr = scenes[name]
        A = make(paths, p_spice, thr, [None if v is None else np.asarray(v, dtype=np.float64) for v in lags], vmin, vmax)
        corr, lags_header = run_steps(A, method)
        ARR[f"{cname}/corr"] = corr
        META["cases"][cname] = {"window": name, "method": method, "small_fov_value_min": vmin,
                                "small_fov_value_max": vmax, "threshold_time": thr,
                                "lags_arcsec": [None if v is None else [float(x) for x in v] for v in lags],
                                "lags_header_units": lags_header, "unit_lag": A.unit_lag}
        print(cname, corr.shape, "nan", int(np.isnan(corr).sum()), "max", np.nanmax(corr) if np.isfinite(corr).any()
              else None, flush=True)
    import astropy
    import scipy
    META["interpreter"] = {"python": sys.version.split()[0], "numpy": np.__version__, "scipy": scipy.__version__,
                           "astropy": astropy.__version__}
    dst = os.path.join(HERE, "iterative_context_golden.npz")
    np.savez_compressed(dst, **ARR)
    with open(os.path.join(HERE, "iterative_context_golden.json"), "w") as f:
        json.dump(META, f, indent=1, sort_keys=True)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
