#!/opt/conda/bin/python3.9
"""
DIFFERENTIAL ROTATION ON THE CARRINGTON PATH, PINNED TO THE REFERENCE'S OWN CODE.

The reference's `Alignment` builds a `DifferentialRotationTransform` for every Carrington resample
(`utils/rectify.py:282-311, 416-423`) but looks the band up with the header's INTEGER `WAVELNTH` in a table with string
keys (`hdrshift/alignment.py:107-108, 891-894`): the lookup never matches, the coefficients become (14.18, 0, 0) and
cancel (quirk Q5).  Here the reference's `align_using_carrington(return_type="corr")` runs with the INSTANCE's table given
the integer keys it lacks, after construction:

    A.rat_wave = {**A.rat_wave, **{int(k): v for k, v in A.rat_wave.items()}}

-- data on the object; no reference statement changes -- which is what `differential_rotation="intended"` computes.
Every case is also run unpatched: the default `differential_rotation="reference"` must keep returning that map.

    tests/golden/diffrot_alignment_golden.npz    the scene pair and the three frames of the jitter session (float32)
    tests/golden/diffrot_alignment_golden.json   headers as astropy read them back, the calls, both maps of every case,
                                                 the corrected header cards of the jitter session

Cases (96^2 / 160^2 `synthetic.make_scene` pair, 72 x 64 grid, 6 h between the images): bands 174 and 304,
`reference_date` defaulted (DATE-AVG of the reference image) and given, a CROTA-lag axis, the parallel branch, a
WAVELNTH outside the table (patched == unpatched), and a 5 x 3 lag plane on which the argmax of the patched map differs
from the unpatched one.  Plus one three-image `jitter_correction_imagers` session, one hour between the frames, its
`Alignment` instances patched the same way.

Run (build container only; about a minute):
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_diffrot_alignment.py
Interpreter and load-time shims: `_reference_loader.py`.  Only reference modules are executed; nothing of them is copied.
"""
import importlib.util
import json
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _reference_loader  # noqa: E402

_reference_loader.load_reference()
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
from astropy.io import fits  # noqa: E402

from euispice_coreg.hdrshift.alignment import Alignment  # noqa: E402
import euispice_coreg.jitter_correction.jitter_correction as ref_jitter  # noqa: E402

spec = importlib.util.spec_from_file_location("coreg_synthetic", os.path.join(ROOT, "euispice_coreg_amd", "synthetic.py"))
synthetic = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synthetic)

STRUCTURAL = {"SIMPLE", "BITPIX", "NAXIS", "EXTEND", "XTENSION", "PCOUNT", "GCOUNT", "END", "COMMENT", "HISTORY", ""}


def _plain(v):
    return v if isinstance(v, (str, bool, int)) else float(v)


def header_as_read(path):
    with fits.open(path) as hdul:
        h = hdul[-1].header
        out = {k: _plain(h[k]) for k in h.keys() if k not in STRUCTURAL and not k.startswith("NAXIS")}
        out["NAXIS1"], out["NAXIS2"] = int(h["NAXIS1"]), int(h["NAXIS2"])
        return out


def write_image(path, img, hdr):
    h = fits.Header()
    for k, v in hdr.items():
        if not k.startswith("NAXIS"):
            h[k] = v
    fits.HDUList([fits.PrimaryHDU(), fits.ImageHDU(data=np.asarray(img, dtype=np.float32), header=h)]).writeto(
        path, overwrite=True)


def patch(A):
    """The integer keys the instance's band table lacks."""
    A.rat_wave = {**A.rat_wave, **{int(k): v for k, v in A.rat_wave.items()}}
    return A


class PatchedAlignment(Alignment):
    """What jitter_correction_imagers constructs, patched as above right after construction."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        patch(self)


def run(ps, pl, call, patched):
    lag = {k: (None if call.get(k) is None else np.asarray(call[k], dtype=np.float64))
           for k in ("lag_crval1", "lag_crval2", "lag_crota")}
    A = Alignment(large_fov_known_pointing=pl, small_fov_to_correct=ps, lag_cdelt1=None, lag_cdelt2=None,
                  parallelism=call["parallelism"], counts_cpu_max=4, reprojection_order=call["order"], **lag)
    if patched:
        patch(A)
    c = A.align_using_carrington(return_type="corr", lonlims=call["lonlims"], latlims=call["latlims"],
                                 shape=call["shape"], reference_date=call["reference_date"])
    return np.asarray(c, dtype=np.float64)[:, :, 0, 0, :, 0]


def main():
    tmp = tempfile.mkdtemp(prefix="golden_diffrot_")
    ARR, META = {}, {"cases": {}, "jitter": {}}
    small, hs, large, hl, _ = synthetic.make_scene(small_n=96, large_n=160, seed=5, n_blobs=120)
    ARR["small"] = np.asarray(small, dtype=np.float32)
    ARR["large"] = np.asarray(large, dtype=np.float32)
    grid = dict(lonlims=[228.0, 262.0], latlims=[-12.0, 22.0], shape=[72, 64])
    l3 = dict(lag_crval1=[13.0, 17.0, 21.0], lag_crval2=[-13.0, -9.0, -5.0], lag_crota=None)
    base = dict(grid, order=2, parallelism=False, reference_date=None, wavelnth=174, date_obs_small="2022-03-17T15:50:45.281")
    cases = {
        # the image to align was taken 6 h after the reference image (DATE-AVG / DATE-OBS 2022-03-17T09:50:45.281)
        "b174_default_date": dict(base, **l3),
        "b304_given_date": dict(base, **l3, wavelnth=304, reference_date="2022-03-17T12:00:00.000"),
        "b304_crota_axis": dict(base, lag_crval1=[13.0, 17.0, 21.0], lag_crval2=[-9.0, -5.0], lag_crota=[-0.3, 0.0, 0.3],
                                wavelnth=304),
        "b174_parallel_order1": dict(base, **l3, parallelism=True, order=1, date_obs_small="2022-03-17T06:50:45.281"),
        "outside_table": dict(base, **l3, wavelnth=1216),
        # 2-arcsec lag step: 6 h of rotation at 304 move the peak by more than one step
        "b304_argmax_moves": dict(base, lag_crval1=[13.0, 15.0, 17.0, 19.0, 21.0], lag_crval2=[-11.0, -9.0, -7.0],
                                  lag_crota=None, wavelnth=304),
    }
    moved = []
    for name, call in cases.items():
        h_s, h_l = dict(hs), dict(hl)
        h_s["DATE-OBS"] = h_s["DATE-AVG"] = call["date_obs_small"]
        h_l["WAVELNTH"] = call["wavelnth"]
        ps, pl = os.path.join(tmp, name + "_small.fits"), os.path.join(tmp, name + "_large.fits")
        write_image(ps, small, h_s)
        write_image(pl, large, h_l)
        maps = {k: run(ps, pl, call, patched=(k == "patched")) for k in ("patched", "unpatched")}
        assert all(np.isfinite(m).all() for m in maps.values()), name
        am = {k: [int(v) for v in np.unravel_index(np.argmax(m), m.shape)] for k, m in maps.items()}
        if am["patched"] != am["unpatched"]:
            moved.append(name)
        META["cases"][name] = {"call": call, "hdr_small": header_as_read(ps), "hdr_large": header_as_read(pl),
                               "patched": maps["patched"].tolist(), "unpatched": maps["unpatched"].tolist(),
                               "argmax_patched": am["patched"], "argmax_unpatched": am["unpatched"]}
        print(name, "argmax patched", am["patched"], "unpatched", am["unpatched"], "max |diff|",
              float(np.abs(maps["patched"] - maps["unpatched"]).max()), flush=True)
    assert np.array_equal(META["cases"]["outside_table"]["patched"], META["cases"]["outside_table"]["unpatched"])
    assert "b304_argmax_moves" in moved, moved
    META["argmax_moves"] = moved

    # ---- a three-image jitter session, one hour between the frames
    series, jit = synthetic.make_series(n_frames=3, n=112, seed=99013, jitter_sigma=3.0, n_blobs=160)
    paths = []
    META["jitter"]["headers"] = []
    for k, (img, h) in enumerate(series):
        h = dict(h)
        h["DATE-OBS"] = h["DATE-AVG"] = "2022-03-17T%02d:50:45.277" % (9 + k)
        ARR[f"frame{k}"] = np.asarray(img, dtype=np.float32)
        p = os.path.join(tmp, f"solo_L2_eui-hrieuv174-image_{k:03d}.fits")
        write_image(p, img, h)
        paths.append(p)
        hr = header_as_read(p)
        del hr["NAXIS1"], hr["NAXIS2"]
        META["jitter"]["headers"].append(hr)
    lag = [float(v) for v in np.arange(-10.0, 10.5, 2.0)]
    call = dict(lonlims=[236.0, 256.0], latlims=[-4.0, 16.0], shape=[88, 88], sublist_length=10, overlap=1,
                parallelism=False)
    META["jitter"]["call"] = dict(call, lag_crval1=lag, lag_crval2=lag)
    META["jitter"]["injected"] = np.asarray(jit).tolist()
    original = ref_jitter.Alignment
    for kind, cls in (("patched", PatchedAlignment), ("unpatched", original)):
        outdir = os.path.join(tmp, "session_" + kind)
        os.makedirs(outdir)
        ref_jitter.Alignment = cls  # the name jitter_correction_imagers constructs its alignments through
        try:
            ref_jitter.jitter_correction_imagers(paths, outdir, lag_crval1=np.asarray(lag), lag_crval2=np.asarray(lag), **call)
        finally:
            ref_jitter.Alignment = original
        outs = []
        for k, p in enumerate(paths):
            with fits.open(os.path.join(outdir, os.path.basename(p))) as f:
                h = f[-1].header
                outs.append({c: float(h[c]) for c in ("CRVAL1", "CRVAL2", "CROTA", "PC1_1", "PC1_2", "PC2_1")})
            print("jitter", kind, "frame", k, outs[-1]["CRVAL1"], outs[-1]["CRVAL2"], "injected", jit[k].tolist(), flush=True)
        META["jitter"]["outputs_" + kind] = outs
    import astropy
    import scipy
    META["interpreter"] = {"python": sys.version.split()[0], "numpy": np.__version__, "scipy": scipy.__version__,
                           "astropy": astropy.__version__}
    dst = os.path.join(HERE, "diffrot_alignment_golden.npz")
    np.savez_compressed(dst, **ARR)
    with open(os.path.join(HERE, "diffrot_alignment_golden.json"), "w") as f:
        json.dump(META, f, indent=1, sort_keys=True)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
