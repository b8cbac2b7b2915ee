"""The case table of the generic k_sweep instantiations (csrc/sweep_variant.hpp): plain data plus the helpers that turn a
row into scenes, oracle maps and GPU sweeps.  tests/test_sweep_variant_cases_cpu.py holds the table to the instantiation
list (every one of the 71 entries is the predicted one of some row here or of a forced pitch of tests/test_gpu_pitch.py);
tests/test_gpu_sweep_variants.py runs every row on the GPU against the oracles.

A row: frame, spline order, float32-exact pixels or not, method, and the options it sets.

  frame           reached through                                    orders -> compiled order
  carrington      sweep_carrington                  (MODE_TRANSLATE)  1, 2, 3; 0, 4, 5 -> run-time order
  helio-series    sweep_helioprojective, h_series 1 (SERIES)          1, 2, 3
  helio-exact     sweep_helioprojective, h_series 0 (HOMOGRAPHY)      1, 2, 3; 0, 4, 5 -> run-time order
  car             sweep_helioprojective on two plate-carree maps      1, 2; 0, 3, 4, 5 -> run-time order

Every run-time-order kernel is driven at all of its orders, so that `order_rt` is a value and not one constant.  Every row
sets "pitch" 0: the automatic pitch would send the common sweeps to the pitched entries (tests/test_gpu_pitch.py's).

Shapes -- the smallest at which the visit kinds of the GPU test occur:
  border    image to align 56 x 64 px, reference 96^2 (tests/test_gpu_pitch.py), 1 % NaN pixels in both; Carrington grid
            40 x 36 over H.CARR_LON / CARR_LAT (partly outside the field of view); helioprojective frames: the sub-map
            semantics, the grid IS the 56 x 64 image, so every lag leaves part of it uncovered; plate carree 60 x 70 on
            90 x 100 (tests/test_gpu_parity.py::test_other_spline_orders_vs_oracle).
  interior  no NaN pixel.  Carrington: the same images, the inner grid of test_method_residus (lon 243-249, lat 2-8:
            every tile (+) lag box inside the image).  Helioprojective: the grid is the image itself, its outer tiles
            always reach the edge, and 56 x 64 is 2 x 2 tiles of 32 x 32 points -- all outer; 96^2 is the smallest square of
            3 x 3 tiles, whose middle one is interior.  Plate carree: the roles' sizes swapped (map to align 90 x 120,
            reference 40 x 48, all of it under the map to align at every lag).
"""
import collections
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import helpers as H
from tests import masked_scores_oracle as M

HERE = os.path.dirname(os.path.abspath(__file__))

# (csrc/sweep_variant.hpp: kTranslate, kHomography, kHomographySeries, kCar; kOrderRt)
TRANSLATE, HOMOGRAPHY, HOMOGRAPHY_SERIES, CAR, ORDER_RT = 0, 1, 2, 3, 0
FIELDS = ("index", "mode", "order", "f32", "round", "resid", "pitch")

# frame -> (mode the sweep asks for, orders the mode compiles, orders it reads at run time, options of its rows)
FRAMES = {
    "carrington": (TRANSLATE, (1, 2, 3), (0, 4, 5), {"pitch": 0}),
    "helio-series": (HOMOGRAPHY_SERIES, (1, 2, 3), (), {"pitch": 0, "h_series": 1}),
    "helio-exact": (HOMOGRAPHY, (1, 2, 3), (0, 4, 5), {"pitch": 0, "h_series": 0}),
    "car": (CAR, (1, 2), (0, 3, 4, 5), {"pitch": 0}),
}
METHODS = ("correlation", "residus_masked")
OPTION_DEFAULTS = {"pitch": -1, "h_series": 1, "use_lds": 1}

Row = collections.namedtuple("Row", "frame order f32_exact method options")


def _rows():
    rows = []
    for frame, (_, compiled, run_time, options) in FRAMES.items():
        for order in compiled + run_time:
            for f32_exact in (True, False):
                for method in METHODS:
                    rows.append(Row(frame, order, f32_exact, method, dict(options)))
    return rows


ROWS = _rows()


def row_id(row):
    return f"{row.frame}-o{row.order}-{'f32' if row.f32_exact else 'f64'}-{row.method}"


def claimed_variant(row):
    """The entry of the instantiation list the row claims to run: (mode, order, f32, round, resid, pitch)."""
    mode, compiled, _, _ = FRAMES[row.frame]
    return (mode, row.order if row.order in compiled else ORDER_RT, row.f32_exact, mode != TRANSLATE,
            row.method != "correlation", 0)


def pick_input(row):
    """What launch_k_sweep hands pick_sweep_variant for the row: (mode, order, f32, residus, pitch asked for)."""
    return (FRAMES[row.frame][0], row.order, int(row.f32_exact), int(row.method != "correlation"), 0)


def has_clean_path(variant):
    """kernels_sweep.hpp kCleanPath: all-finite interior visits drop the sample mask."""
    mode, order, f32, rnd, resid, _ = variant
    return mode != CAR and not resid and order != ORDER_RT and not (rnd and not f32)


# ---- the pick, by the library's own header on the host -------------------------------------------------------------
def _compiler():
    for cc in ("g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if shutil.which(cc):
            return cc
    return None


def have_compiler():
    return _compiler() is not None


@functools.lru_cache(maxsize=None)
def _pick_program():
    exe = os.path.join(tempfile.mkdtemp(prefix="sweep_variant_pick_"), "sweep_variant_pick")
    cc = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                         os.path.join(HERE, "native", "sweep_variant_pick.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    return exe


def native_picks(inputs):
    """(entries, indices): the instantiation list as tuples (mode, order, f32, round, resid, pitch), and for every
    (mode, order, f32, residus, pitch) of `inputs` the index pick_sweep_variant gives it."""
    text = "".join("%d %d %d %d %d\n" % tuple(int(v) for v in i) for i in inputs)
    r = subprocess.run([_pick_program()], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    entries, picks = [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "entry":
            assert int(w[1]) == len(entries)
            m, o, f, rd, rs, p = (int(v) for v in w[2:])
            entries.append((m, o, bool(f), bool(rd), bool(rs), p))
        else:
            picks.append(int(w[1]))
    assert len(picks) == len(inputs)
    return entries, picks


@functools.lru_cache(maxsize=None)
def predicted():
    """row id -> index of the instantiation the row runs."""
    _, picks = native_picks([pick_input(r) for r in ROWS])
    return {row_id(r): p for r, p in zip(ROWS, picks)}


# ---- scenes ---------------------------------------------------------------------------------------------------------
GEOMETRIES = ("border", "interior")
PX1, PX2 = 1007.616 / 64, 1007.616 / 56  # arcsec per pixel of the 56 x 64 image (synthetic.make_scene)
BORDER_GRID = dict(shape=(40, 36), lonlims=H.CARR_LON, latlims=H.CARR_LAT)
INNER_GRID = dict(shape=(40, 36), lonlims=(243.0, 249.0), latlims=(2.0, 8.0))
HELIO_INTERIOR_N = 96


def _not_float32_exact(img):
    return np.asarray(img, dtype=np.float64) + 1e-9 * np.arange(img.size).reshape(img.shape)


@functools.lru_cache(maxsize=None)
def scene(frame, f32_exact, geometry):
    """dict: small, hs, large, hl, lags (the five lists) and, on the Carrington frame, grid (shape, lonlims, latlims)."""
    nan_frac = 0.01 if geometry == "border" else 0.0
    rng = np.random.default_rng(11)
    if frame == "car":
        from euispice_coreg_amd import synthetic
        shapes = dict(small_shape=(60, 70), large_shape=(90, 100)) if geometry == "border" else \
            dict(small_shape=(90, 120), large_shape=(40, 48))
        small, hs, large, hl, _ = synthetic.make_car_scene(nan_frac=nan_frac, **shapes)
        if nan_frac:
            large = large.copy()
            large[rng.random(large.shape) < nan_frac] = np.nan
        small = small if f32_exact else _not_float32_exact(small)  # (float32 pixels: made inexact as test_gpu_upload does)
        lags = (np.array([0.0, 0.018]), np.array([-0.011, 0.004]), None, None, None)  # degrees, ~2 px apart
        return dict(small=small, hs=hs, large=large, hl=hl, lags=lags)
    if frame == "carrington" or geometry == "border":
        small, hs, large, hl, _ = H.scene(small_shape=(56, 64), large_n=96, float32_exact=f32_exact, nan_frac=nan_frac)
        px1, px2 = PX1, PX2
    else:
        n = HELIO_INTERIOR_N
        small, hs, large, hl, _ = H.scene(small_n=n, large_n=128, float32_exact=f32_exact, nan_frac=nan_frac)
        px1 = px2 = 1007.616 / n
    if nan_frac:
        large = large.copy()
        large[rng.random(large.shape) < nan_frac] = np.nan
    if frame == "carrington":  # +-1 px about the scene's pointing error
        c1, c2 = 17.0 + px1 * np.arange(-1, 2), -9.0 + px2 * np.arange(-1, 2)
    elif geometry == "border":  # through exactly 0.0 on both axes: the zero lag's border, parity and tap passes
        c1, c2 = px1 * np.arange(-1.0, 2.0), px2 * np.arange(-1.0, 2.0)
    else:
        c1, c2 = 17.0 + px1 * np.array([-1.0, 1.0]), -9.0 + px2 * np.array([-1.0, 1.0])
    out = dict(small=small, hs=hs, large=large, hl=hl, lags=(c1, c2, None, None, np.array([0.0, 0.3])))
    if frame == "carrington":
        out["grid"] = BORDER_GRID if geometry == "border" else INNER_GRID
    return out


# ---- the oracles ------------------------------------------------------------------------------------------------------
def _state(frame, order, sc):
    if frame == "carrington":
        g = sc["grid"]
        return H.oracle_state(sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"], order=order, shape=list(g["shape"]),
                              lonlims=list(g["lonlims"]), latlims=list(g["latlims"]), solar_r=(1.004,))
    return H.oracle_state(sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"], order=order,
                          unit_lag="deg" if frame == "car" else "arcsec")


def oracle_correlation(frame, order, f32_exact, geometry):
    """H.oracle_carrington / H.oracle_helio (plate carree: the full-grid semantics, lags in degrees)."""
    sc = scene(frame, f32_exact, geometry)
    a = (sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"])
    if frame == "carrington":
        return H.oracle_carrington(*a, order=order, **sc["grid"])
    if frame == "car":
        return H.oracle_helio(*a, order=order, parallelism=False, unit_lag="deg")
    return H.oracle_helio(*a, order=order)


def oracle_masked(frame, order, f32_exact, geometry):
    """tests/masked_scores_oracle.sweep: the masked residus and both kinds of counts."""
    sc = scene(frame, f32_exact, geometry)
    st = _state(frame, order, sc)
    if frame == "carrington":
        return M.sweep(st, "carrington")
    return M.sweep(st, "helioprojective", parallelism=frame != "car")


def oracle_plain_residus(order, f32_exact):
    """Plain 'residus' on the Carrington frame's full-overlap grid."""
    from oracle import coreg_oracle as O
    return O.find_best_header_parameters(_state("carrington", order, scene("carrington", f32_exact, "interior")),
                                         "carrington", method="residus")


# ---- the GPU side ---------------------------------------------------------------------------------------------------
def method_code(method):
    from euispice_coreg_amd import _lib
    return {"correlation": _lib.METHOD_CORRELATION, "residus_masked": _lib.METHOD_RESIDUS_MASKED,
            "residus": _lib.METHOD_RESIDUS}[method]


def gpu_prepare(h, row, geometry):
    """Uploads the row's images and prepares its reference; returns a function (method, use_lds) -> 6-D map."""
    from euispice_coreg_amd import _lib
    sc = scene(row.frame, row.f32_exact, geometry)
    ls = _lib.LagSet(*sc["lags"])
    h.set_small(sc["small"])
    if row.frame == "carrington":
        grid = _lib.Grid(sc["grid"]["lonlims"], sc["grid"]["latlims"], sc["grid"]["shape"])
        h.prepare_reference_carrington(sc["large"], sc["hl"], grid, 1.004, row.order)
    elif row.frame == "car":
        h.set_reference_on_grid(np.asarray(sc["large"], dtype=np.float32))
    else:
        h.prepare_reference_helioprojective(sc["large"], sc["hl"], sc["hs"], row.order)

    def sweep(method, use_lds=1):
        try:
            for name, value in dict(row.options, use_lds=use_lds).items():
                h.set_option(name, value)
            if row.frame == "carrington":
                out = h.sweep_carrington(sc["hs"], grid, 1.004, ls, order=row.order, method=method_code(method))
            else:
                target = sc["hl"] if row.frame == "car" else sc["hs"]
                out = h.sweep_helioprojective(target, sc["hs"], ls, order=row.order, method=method_code(method))
        finally:
            for name, value in OPTION_DEFAULTS.items():
                h.set_option(name, value)
        return out.reshape(ls.shape + (1,))

    return sweep
