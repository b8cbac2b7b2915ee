"""
The job catalogue of tests/test_gpu_handle_history.py: small, self-contained units of work on a `CoregHandle`, one per
kind of state the handle keeps (host_state.hpp, ContextState, PixelsState).  Importable without a GPU: a job's inputs
are built on first use and kept, nothing here touches the device until a job is called with a handle.

A job is `setup(h)` -- every call it needs from `set_small` onwards, every sticky setting it depends on set, None
included, as the classes do (hdrshift/alignment.py: "the handle is long-lived and keeps its rotations") -- and
`run(h) -> {name: ndarray}`, what is compared bit for bit between a fresh handle and one with a past: the score map,
the sample counts and, where it costs one read-back, the resident images.  A job leaves its sticky settings SET when it
returns (the next job has to clear what it does not want); only options (`set_option`) are restored, as every test of
the suite restores them.

`check(out)` compares a fresh result with the CPU oracle of that path at the tolerance of the existing test named in
`cites`; no tolerance is introduced here.

Sizes: images of 24 to 96 px on a side, 2 x 2 to 5 x 5 CRVAL lags, grids of 32 x 32 or smaller; consecutive jobs of the
catalogue differ in image shape, grid shape and lag count, so every buffer that only grows is also used smaller than
it is.
"""
from functools import lru_cache

import numpy as np

from euispice_coreg_amd import _lib
from tests import helpers as H

CORR, RESIDUS, MASKED, MI = (_lib.METHOD_CORRELATION, _lib.METHOD_RESIDUS, _lib.METHOD_RESIDUS_MASKED,
                             _lib.METHOD_MUTUAL_INFORMATION)
SOLAR_R = 1.004
ROT = (2.0, 14.51, -3.12, 0.34)  # days, then the three coefficients in degrees per day (tests/test_gpu_diffrot.py)
INNER = dict(lon=(243.0, 249.0), lat=(2.0, 8.0))  # a grid inside the field of view for every lag (test_method_residus)


class Job:
    def __init__(self, name, family, size, setup, run, check, cites, refusal=False):
        self.name, self.family, self.size, self.refusal = name, family, size, refusal
        self.setup, self.run, self.check, self.cites = setup, run, check, cites

    def __call__(self, h):
        self.setup(h)
        return self.run(h)

    def __repr__(self):
        return f"Job({self.name})"


def lags2(n1, n2, step=2.0, c1=17.0, c2=-9.0, cdelt1=None, cdelt2=None, crota=None):
    return (c1 + step * (np.arange(n1) - n1 // 2), c2 + step * (np.arange(n2) - n2 // 2), cdelt1, cdelt2, crota)


def n_lags(lags):
    return int(np.prod([1 if v is None else len(v) for v in lags]))


# ---- scenes (built once) --------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def scene(small_shape, large_n, seed=5, f32=True, nan_frac=0.005):
    return H.scene(small_shape=small_shape, large_n=large_n, seed=seed, float32_exact=f32, nan_frac=nan_frac)[:4]


def with_spikes(v, seed, every=60, lo=300.0, hi=5000.0):
    """`v` with one pixel in `every` raised by a whole number in [lo, hi) (float32-exact pixels stay so)."""
    rng = np.random.default_rng(seed)
    out = np.array(v, copy=True)
    at = rng.choice(out.size, size=max(4, out.size // every), replace=False)
    out.ravel()[at] += np.round(rng.uniform(lo, hi, at.size))
    return out


def gauss(r):
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * (r / 4.0) ** 2))
    return w / w.sum()


def lopsided(r, seed):
    w = np.random.default_rng(seed).uniform(0.0, 1.0, 2 * r + 1)
    w[: r // 2] *= 3.0
    return w / w.sum()


SMALL_TABLES = (gauss(4), lopsided(3, 9))   # the image to align
REF_TABLES = (lopsided(3, 8), gauss(5))     # the reference image
SMALL_RULE = dict(radius=2, n_iter=2, nsigma=5.0, min_neighbours=5, sign="positive", replace="nan", floor=0.0)
REF_RULE = dict(radius=3, n_iter=2, nsigma=4.0, min_neighbours=5, sign="both", replace="median", floor=0.0)


# ---- Carrington sweeps ------------------------------------------------------------------------------------------------
def _visits(h):
    c = h.last_visit_counts()
    return np.array([c["refined_lag_points"], c["flagged_not_refined"]], dtype=np.int64)


def carr_job(name, get_scene, shape, lags, order=2, method=CORR, rot=(None, None), smooth=None, despike=None,
             small_ops=None, bins=None, lon=H.CARR_LON, lat=H.CARR_LAT, atol=1e-10, check=None, cites=None,
             oracle_images=None, shard=None, expect_refined=None, n_lags_hint=1):
    """One Carrington sweep.  small_ops: (vmax, despike rule, smoothing tables) applied to the resident image to align,
    in that order, each None for "not applied".  bins: a function -> (edges_small, edges_large).  oracle_images: a
    function -> (small, large) as the oracle must see them (the CPU restatement of what the device did to them).
    shard: the number of grid shares swept one after the other and added (coreg_finalize_sums)."""
    grid = _lib.Grid(lon, lat, shape)

    def the_lags():
        return lags() if callable(lags) else lags

    def setup(h):
        small, hs, large, hl = get_scene()
        h.set_point_shard(0, 1)
        h.set_rotation("reference", rot[0])
        h.set_rotation("small", rot[1])
        h.set_reference_smoothing(smooth)
        h.set_reference_despike(despike)
        h.set_small(small)
        if small_ops is not None:
            vmax, rule, tables = small_ops
            if vmax is not None:
                h.threshold_small(None, vmax)
            if rule is not None:
                h.despike_small(rule)
            if tables is not None:
                h.smooth_small(tables)
        h.prepare_reference_carrington(large, hl, grid, SOLAR_R, order)
        if bins is not None:
            h.sweep_set_bins(*bins())

    def run(h):
        small, hs, large, hl = get_scene()
        ls = _lib.LagSet(*the_lags())
        if shard is None:
            out = h.sweep_carrington(hs, grid, SOLAR_R, ls, order=order, method=method)
        else:
            total = None
            try:
                for r in range(shard):
                    h.set_point_shard(r, shard)
                    h.sweep_carrington(hs, grid, SOLAR_R, ls, order=order, method=method)
                    part = h.copy_sums()
                    total = part if total is None else total + part
                out = h.finalize_sums(total, ls.size)
            finally:
                h.set_point_shard(0, 1)
        return dict(map=out, counts=h.last_counts(), visits=_visits(h), small=h.get_small(np.shape(small)),
                    ref=h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64))

    def default_check(out):
        small, hs, large, hl = get_scene()
        if oracle_images is not None:
            small, large = oracle_images()
        want = H.oracle_carrington(small, hs, large, hl, the_lags(), shape, lonlims=lon, latlims=lat, order=order)
        assert np.isfinite(want).any()
        H.assert_corr_close(out["map"].reshape(want.shape), want, atol, name)
        if expect_refined is not None:
            assert (out["visits"][0] > 0) == expect_refined, out["visits"]

    size = shape[0] * shape[1] * (n_lags_hint if callable(lags) else n_lags(lags))
    return Job(name, "carrington", size, setup, run, check or default_check,
               cites or "tests/test_gpu_parity.py::test_sweep_carrington_vs_oracle (1e-10)")


def _sc_a():
    return scene((64, 64), 96)


def _sc_b():
    return scene((40, 56), 80, seed=6)


def _sc_f64():
    return scene((48, 48), 72, seed=7, f32=False)


def _sc_full():
    return scene((64, 64), 96, seed=5, nan_frac=0.0)


@lru_cache(maxsize=None)
def _sc_spiked():
    small, hs, large, hl = scene((56, 48), 88, seed=8)
    large = with_spikes(large, 37)
    large[40:43, 30:50] = np.nan  # a hole the taps must not spread
    return with_spikes(small, 31), hs, large, hl


@lru_cache(maxsize=None)
def _ref_images(smooth, despike):
    from tests import despike_oracle as DO
    from tests import smooth_oracle as SO
    small, hs, large, hl = _sc_spiked()
    if despike:
        large = DO.despike(large, **REF_RULE)[0]
    if smooth:
        large = SO.smooth(large, *REF_TABLES)
    return small, large


VMAX = 2500.0


@lru_cache(maxsize=None)
def _small_images(ops):
    from euispice_coreg_amd.utils import header as hdrutil
    from tests import despike_oracle as DO
    from tests import smooth_oracle as SO
    small, hs, large, hl = _sc_spiked()
    if ops:
        small = small.copy()
        hdrutil.set_threshold_minmax_to_nan(small, None, VMAX)
        assert np.isnan(small).sum() > np.isnan(_sc_spiked()[0]).sum()
        small, counts = DO.despike(small, **SMALL_RULE)
        small = SO.smooth(small, *SMALL_TABLES)
    return small, large


@lru_cache(maxsize=None)
def _random_80246():
    """Six active grid points, lag-points whose coefficient is +-1 by construction (tests/deep_fuzz.py seed 80246)."""
    from tests.test_gpu_fuzz import _random_case
    small, hs, large, hl, lags, _ = _random_case(80246)
    lags = list(lags)
    lags[3] = [0.0, -0.02]
    return (small, hs, large, hl), tuple(None if v is None else tuple(np.asarray(v, dtype=np.float64)) for v in lags)


def _refine_job():
    def lags():
        return tuple(None if v is None else np.array(v) for v in _random_80246()[1])
    return carr_job("carr_refine", lambda: _random_80246()[0], (23, 25), lags, lon=(200.0, 234.0), lat=(-72.0, 22.0),
                    atol=1e-13, expect_refined=True, n_lags_hint=20,
                    cites="tests/test_gpu_parity.py::test_ill_conditioned_lag_points_are_re_evaluated_with_centred_sums (1e-13)")


# ---- mutual information, residus ----------------------------------------------------------------------------------------
def _mi_state(get_scene, lags, shape, order=2):
    from tests.test_gpu_masked_scores import carr_state
    small, hs, large, hl = get_scene()
    st = carr_state(small, hs, large, hl, lags, shape)
    st.order = order
    return st


@lru_cache(maxsize=None)
def _mi_edges(which):
    """(edges_small, edges_large): quantile edges of the image to align and of the oracle's reference on the grid."""
    from euispice_coreg_amd.pxlshift.alignment_pixels import quantile_edges
    from oracle import coreg_oracle as O
    get_scene, shape, n_small, n_large = MI_CASES[which][:4]
    ref = O.prepare_reference(_mi_state(get_scene, lags2(1, 1), shape), "carrington", SOLAR_R, True)
    return quantile_edges(get_scene()[0], n_small), quantile_edges(ref, n_large)


MI_CASES = {"mi_8x8_5x5": (_sc_a, (32, 28), 8, 8, lags2(5, 5)), "mi_4x12_3x3": (_sc_b, (22, 26), 4, 12, lags2(3, 3))}


def mi_job(name):
    get_scene, shape, _, _, lags = MI_CASES[name]

    def check(out):
        from tests import hdrshift_mi_oracle as MO
        from tests.test_gpu_hdrshift_mi import BOUND_MARGIN, EDGE_MARGIN, _check
        es, el = _mi_edges(name)
        edge, bound = MO.margins(_mi_state(get_scene, lags, shape), es, el)
        assert edge > EDGE_MARGIN and bound > BOUND_MARGIN, (name, edge, bound)
        want = MO.sweep(_mi_state(get_scene, lags, shape), "carrington", es, el)
        _check(out["map"], out["counts"], {k: v.ravel() for k, v in want.items()}, name)

    return carr_job(name, get_scene, shape, lags, method=MI, bins=lambda: _mi_edges(name), check=check,
                    cites="tests/test_gpu_hdrshift_mi.py::test_usual_grid (equal counts, 1e-11)")


def residus_job():
    shape, lags = (30, 26), lags2(3, 3)

    def check(out):
        from oracle import coreg_oracle as O
        small, hs, large, hl = _sc_full()
        st = H.oracle_state(small, hs, large, hl, lags, shape=list(shape), lonlims=list(INNER["lon"]),
                            latlims=list(INNER["lat"]), solar_r=(SOLAR_R,))
        want = O.find_best_header_parameters(st, "carrington", method="residus")
        assert np.isfinite(want).all()
        got = out["map"].reshape(want.shape)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        assert np.argmin(got) == np.argmin(want)

    return carr_job("carr_residus", _sc_full, shape, lags, method=RESIDUS, check=check, **INNER,
                    cites="tests/test_gpu_parity.py::test_method_residus (1e-10 relative)")


def masked_job():
    shape, lags = (26, 30), lags2(4, 3)

    def check(out):
        from tests import masked_scores_oracle as M
        from tests.test_gpu_masked_scores import CARR_RTOL, assert_counts, assert_masked, carr_state
        small, hs, large, hl = _sc_a()
        want = M.sweep(carr_state(small, hs, large, hl, lags, shape), "carrington")
        assert_counts(out["counts"], want["finite_terms"], "carr_residus_masked")
        assert_masked(out["map"], want["masked"], CARR_RTOL, "carr_residus_masked")

    return carr_job("carr_residus_masked", _sc_a, shape, lags, method=MASKED, check=check,
                    cites="tests/test_gpu_masked_scores.py::test_carrington_usual_grid (equal counts, 1e-10)")


def rot_job():
    """Both rotations set.  The CPU oracle has no differential rotation (the rotated resample is held to the reference's
    own output by tests/test_gpu_diffrot.py): (b) for this job is that the map is finite and is NOT its twin's."""
    shape, lags = (28, 24), lags2(3, 4)

    def check(out):
        small, hs, large, hl = _sc_a()
        plain = H.oracle_carrington(small, hs, large, hl, lags, shape)
        assert np.isfinite(out["map"]).all() and np.abs(out["map"].reshape(plain.shape) - plain).max() > 1e-6

    return carr_job("carr_rot_both", _sc_a, shape, lags, rot=(ROT, ROT), check=check,
                    cites="tests/test_gpu_diffrot.py::test_rotation_set_then_cleared_equals_an_untouched_handle")


# ---- helioprojective and plate-carree sweeps ------------------------------------------------------------------------------
def helio_job(name, get_scene, px, lags, order=2, serial=False, options=(), combo=None, atol=1e-7, cites=None,
              unit="arcsec"):
    """px: the pixels of the image to align (orders by size).  options: ((name, value, default), ...) set for the sweep
    and restored.  combo: (begin, end) of the (cdelt1, cdelt2,
    crota) combinations, the one-shot options of the next sweep."""
    ls = _lib.LagSet(*lags)
    inner = ls.shape[2] * ls.shape[3] * ls.shape[4]

    def setup(h):
        small, hs, large, hl = get_scene()
        h.set_point_shard(0, 1)
        h.set_reference_smoothing(None)
        h.set_reference_despike(None)
        h.set_small(small)
        if serial:
            h.set_reference_on_grid(np.asarray(large, dtype=np.float64 if serial == "f64" else np.float32))
        else:
            h.prepare_reference_helioprojective(large, hl, hs, order)

    def run(h):
        small, hs, large, hl = get_scene()
        target = hl if serial else hs
        for opt, value, _ in options:
            h.set_option(opt, value)
        try:
            if combo is None:
                out = h.sweep_helioprojective(target, hs, ls, order=order)
            else:
                h.set_option("combo_begin", combo[0])
                h.set_option("combo_end", combo[1])
                out = h.sweep_helioprojective(target, hs, ls, order=order, lag_begin=0,
                                              lag_end=ls.shape[0] * ls.shape[1] * (combo[1] - combo[0]))
        finally:
            for opt, _, default in options:
                h.set_option(opt, default)
        t = h.last_tap_fix()
        ref_shape = np.shape(large) if serial else np.shape(small)
        return dict(map=out, counts=h.last_counts(), visits=_visits(h),
                    tap=np.array([t["samples"], t["lag_points"], t["overflow"]], dtype=np.int64),
                    small=h.get_small(np.shape(small)),
                    ref=h.get_reference_on_grid(ref_shape, np.float64 if serial == "f64" else np.float32))

    def check(out):
        small, hs, large, hl = get_scene()
        want = H.oracle_helio(np.asarray(small, dtype=np.float64), hs, np.asarray(large, dtype=np.float64), hl, lags,
                              order=order, parallelism=not serial, unit_lag=unit)
        assert np.isfinite(want).any()
        if combo is not None:
            want = want.reshape(ls.shape[0], ls.shape[1], inner)[:, :, combo[0]:combo[1]]
        H.assert_corr_close(out["map"].reshape(want.shape), want, atol, name)

    return Job(name, "helioprojective", px * ls.size, setup, run, check,
               cites or "tests/test_gpu_parity.py::test_sweep_helioprojective_vs_oracle (1e-7)")


def _sc_h1():
    return scene((50, 50), 96, seed=4, f32=False, nan_frac=0.02)


def _sc_h3():
    return scene((44, 36), 80, seed=6, nan_frac=0.02)


def _sc_h2():
    return scene((64, 64), 96)


ZERO_LAGS = (np.array([-4.0, 0.0, 4.0]), np.array([0.0, -3.0]), [0.0, 0.03], None, [0.0, 0.5])
LAGS_5D = (np.array([15.0, 17.0, 19.0]), np.array([-11.0, -9.0, -7.0]), [0.0, 0.05], [0.0, -0.04], [0.0, 0.5])
CDELT1_70 = 0.002 * (np.arange(70) - 20.0)  # 70 distinct CDELT1 lags, the identity among them
LAGS_70 = (np.array([0.0]), np.array([0.0]), CDELT1_70, None, None)
# the same lags, last first: the border-pixel cache is cleared at 64 entries and the tap-flag cache at 4, so what a sweep
# of LAGS_70 leaves behind are its LAST lags -- a sweep that begins with them meets them before it has evicted them
LAGS_70_REVERSED = (np.array([0.0]), np.array([0.0]), CDELT1_70[::-1].copy(), None, None)


def _sc_48():
    return scene((48, 48), 72, seed=3, nan_frac=0.01)


@lru_cache(maxsize=None)
def _sc_48_in_56():
    """The header cards of `_sc_48` on BOTH sides: a 48 x 48 reference on the grid of that header, and a 56 x 56 image to
    align whose header differs from it in NAXIS alone.  The lag-points of LAGS_70 then have the target and shifted cards
    of the job on `_sc_48` and the same grid -- only the size of the image to align, which decides the bounds rule, is
    another: a cache of the host's wcslib passes that forgot that size would hand this job the other one's pixels (21 of
    the 48 pixels of row 47, which the round trip sends above 47: the last row there, an inner row here)."""
    small48, hs48, _, _ = _sc_48()
    small56 = scene((56, 56), 72, seed=9, nan_frac=0.01)[0]
    ref = np.nan_to_num(scene((48, 48), 72, seed=11)[0], nan=150.0)
    hs56 = dict(hs48, NAXIS1=56, NAXIS2=56)
    return small56, hs56, ref, dict(hs48)


@lru_cache(maxsize=None)
def _sc_car():
    from euispice_coreg_amd import synthetic
    cs, chs, cl, chl, _ = synthetic.make_car_scene(small_shape=(60, 70), large_shape=(90, 100))
    return cs, chs, cl, chl


CAR_LAGS = (np.array([0.0, 0.018]), np.array([-0.011, 0.004]), None, None, None)


# ---- iterative context ----------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _context_case(which):
    from tests import context_cases as CC
    three = np.array([-2.0, 0.0, 2.0]) * CC.AS
    if which == 0:
        return CC.make_case(7, gW=5, gH=7, method="correlation", order=2, n_frames=2, col_mode="every",
                            thresholds="none", nan_frac=0.0, frame_dtype=np.float32, spice_dtype=np.float64,
                            lags=[three, three, None, None, None])
    return CC.make_case(6001, gW=12, gH=30, method="correlation", order=2, n_frames=3, col_mode="random",
                        thresholds="min", nan_frac=0.01, frame_dtype=np.float64, spice_dtype=np.float32,
                        lags=[three[:2], three, None, None, np.array([0.0, 0.4])])


def context_job(name, which):
    def setup(h):
        from tests import context_cases as CC
        CC.upload(h, _context_case(which))

    def run(h):
        from tests import context_cases as CC
        out = CC.gpu(h, _context_case(which), upload_first=False)
        return dict(map=out, counts=h.last_counts())

    def check(out):
        from tests import context_cases as CC
        from tests.test_gpu_context_fuzz import assert_matches
        assert_matches(out["map"], CC.oracle(_context_case(which)), "correlation", name)

    return Job(name, "context", 100 * (which + 1), setup, run, check,
               "tests/test_gpu_context_fuzz.py::test_handle_reuse_across_scenes (1e-8)")


# ---- pixel-lag sweeps -------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _pixels(which):
    """(AlignmentPixels on in-memory arrays, keyword arguments of its plan)."""
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    from tests import pxlshift_mi_oracle as M
    from tests.pxlshift_tiles_cases import HDR, two_drift_scene
    if which == "mi_scene":
        large, small, _ = M.scene(seed=1, shape=(24, 20), lag=(-1, 1))
        kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    elif which == "mi_scene_b":
        large, small, _ = M.scene(seed=2, shape=(28, 34), lag=(1, -2))
        kw = dict(lag_dx=np.arange(-3, 4), lag_dy=np.arange(-2, 3), lag_drot=np.array([0.0]))
    else:
        large, small, _, _, _ = two_drift_scene()
        kw = dict(lag_dx=np.arange(-2, 3), lag_dy=np.arange(-2, 3), lag_drot=np.array([0.0]))
    return AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0), kw


PIXELS_SIZE = {"mi_scene": 24 * 20 * 15, "mi_scene_b": 28 * 34 * 35, "drift": 40 * 48 * 25}


def pixels_job(name, which, mode="plain", method="correlation", shift=None, tile=None, step=None, bins=None, cites=None):
    def plan_of():
        A, kw = _pixels(which)
        more = {}
        if tile is not None:
            more["tile_shape"] = tile
        if step is not None:
            more["tile_step"] = step
        if bins is not None:
            more["bins"] = bins
        return A, A.host_plan(**kw, method=method, **more)

    def setup(h):
        A, plan = plan_of()
        h.pixels_set_large(A.data_large)
        h.pixels_set_small(A.data_small)
        if shift is not None:
            h.pixels_shift_large(*shift)

    def run(h):
        A, plan = plan_of()
        code = plan["method_code"]
        if mode == "plain":
            cube = h.pixels_sweep(plan, code)
            counts = h.pixels_last_counts(cube.shape)
        elif mode == "tiles":
            cube = h.pixels_sweep_tiles(plan, code)
            counts = h.pixels_last_tile_counts(cube.shape)
        else:
            cube = h.pixels_sweep_windows(plan, code, tile, step)
            counts = h.pixels_last_tile_counts(cube.shape)
        n_dx, n_dy = len(plan["lag_dx"]), len(plan["lag_dy"])
        hh, ww = A.data_small.shape
        return dict(map=cube, counts=counts, large=h.pixels_get_image("large", A.data_large.shape),
                    small=h.pixels_get_image("small", A.data_small.shape),
                    box=h.pixels_get_large_box((hh + int(np.ptp(plan["lag_dy"])), ww + int(np.ptp(plan["lag_dx"])))),
                    plane=h.pixels_get_rotated(0, A.data_small.shape))

    def check(out):
        A, plan = plan_of()
        if shift is not None:
            plan = dict(plan, shift_large=shift)
        if method == "mutual_information":
            from tests import pxlshift_mi_oracle as M
            from tests.test_gpu_pxlshift_mi import _check
            o = M.scores(None, A.data_small, plan, planes=[out["plane"]], box=out["box"])
            _check(out["map"], o["mi"], out["counts"], o["count"], name)
        elif mode == "plain":
            from tests import pxlshift_scores_oracle as S
            from tests.test_gpu_pxlshift_scores import _check_corr, _check_masked
            o = S.scores(A.data_large, A.data_small, plan)
            if method == "correlation":
                assert np.array_equal(out["counts"], o["count"])
                _check_corr(out["map"], o["corr"], name)
            else:
                assert np.array_equal(out["counts"], o["finite_terms"])
                _check_masked(out["map"], o["masked"], name)
        elif mode == "tiles":
            from tests import pxlshift_tiles_oracle as T
            from tests.test_gpu_pxlshift_tiles import _check
            o = T.scores(A.data_large, A.data_small, plan, tile)
            assert np.array_equal(out["counts"], o["count"])
            _check(out["map"], o["corr"], "correlation", name, ties=True)
        else:
            from tests import pxlshift_windows_oracle as W
            from tests.test_gpu_pxlshift_windows import _check
            o = W.scores(A.data_large, A.data_small, plan, tile, step)
            assert np.array_equal(out["counts"], o["count"])
            _check(out["map"], o["corr"], "correlation", name, ties=True)

    return Job(name, "pixels", PIXELS_SIZE[which], setup, run, check,
               cites or "tests/test_gpu_pxlshift_scores.py::test_counts_and_scores_against_the_oracle "
                        "(equal counts, 2^-23 |corr| + 1e-12)")


@lru_cache(maxsize=None)
def _destretch_inputs():
    rng = np.random.default_rng(41)
    ny, nx, tile = 21, 30, (10, 16)
    cube = rng.uniform(1.0, 9.0, (2, ny, nx)).astype(np.float32)
    cube[rng.integers(0, 2, 9), rng.integers(0, ny, 9), rng.integers(0, nx, 9)] = np.nan

    def centres(n, t):
        return np.array([(a + min(n, a + t) - 1) / 2 for a in range(0, n, t)], dtype=np.float64)
    ys, xs = centres(ny, tile[0]), centres(nx, tile[1])
    u, v = rng.uniform(-3, 3, (len(ys), len(xs))), rng.uniform(-3, 3, (len(ys), len(xs)))
    return cube, ys, xs, u, v, tile


def destretch_job():
    def run(h):
        cube, ys, xs, u, v, tile = _destretch_inputs()
        out, disp = h.pixels_destretch(cube, ys, xs, u, v, tile, 0, return_displacement=True)
        return dict(planes=out, displacement=disp)

    def check(out):
        from tests import pxlshift_destretch_oracle as D
        from tests.test_gpu_pxlshift_destretch import _same_bits
        cube, ys, xs, u, v, tile = _destretch_inputs()
        want, wd = D.destretch(cube, ys, xs, u, v, tile, "bilinear")
        assert _same_bits(out["displacement"], wd) and _same_bits(out["planes"], want)
        assert 0 < np.isnan(want).sum() < want.size

    return Job("pix_destretch", "pixels", 2 * 21 * 30, lambda h: None, run, check,
               "tests/test_gpu_pxlshift_destretch.py::test_an_image_of_several_workgroups (the oracle's bits)")


# ---- despiked plane sums ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _stack(n, shape, seed, f32):
    rng = np.random.default_rng(seed)
    full = (n,) + tuple(shape)
    v = 100.0 + rng.normal(0.0, 1.0, full)
    hit = rng.uniform(size=full) < 0.09
    v[hit] += rng.uniform(20.0, 4000.0, int(hit.sum()))
    v[rng.uniform(size=full) < 0.03] -= 60.0
    return v.astype(np.float32) if f32 else v + 1e-9 * np.pi


PLANES_RULE = dict(radius=2, n_iter=2, min_neighbours=5)


def planes_job(name, n, shape, seed, f32):
    def run(h):
        from tests import despike_planes_oracle as PO
        s, events, counts = h.despike_sum_planes(PO.be(_stack(n, shape, seed, f32)), np.arange(n), PLANES_RULE)
        return dict(sum=s, events=events, flagged=np.array(counts, dtype=np.int64))

    def check(out):
        from tests import despike_planes_oracle as PO
        want_sum, want_events, want_counts = PO.despike_sum_planes(_stack(n, shape, seed, f32), **PLANES_RULE)
        assert out["flagged"].tolist() == want_counts and sum(want_counts) > 0
        assert np.array_equal(out["events"], want_events)
        assert np.array_equal(out["sum"], want_sum, equal_nan=True)

    return Job(name, "planes", n * shape[0] * shape[1], lambda h: None, run, check,
               "tests/test_gpu_despike_planes.py::test_planes_against_the_oracle (the oracle's bits)")


# ---- refused calls (every one a host-side check that returns before any launch) ---------------------------------------------
def refusal_job(name, family, call, code):
    """`call(h)` must raise CoregError with `code`; what is compared is the code.  The checks behind them, in the order
    the library makes them: abi_sweeps.hpp open_sweep (check_method, check_order, check_wcs / check_grid, check_lags: all
    before bind_device and begin_sweep), coreg_finalize_sums ("no point-sharded sweep is pending", its first statement),
    host_despike_planes.hpp ("before any GPU work: a refused call changes nothing"), coreg_set_option (the last else)
    and sweep_mi_set_bins (the lists are checked before they are stored)."""
    def run(h):
        try:
            call(h)
        except _lib.CoregError as e:
            return dict(code=np.array([e.code], dtype=np.int64))
        return dict(code=np.array([_lib.COREG_OK], dtype=np.int64))

    def check(out):
        assert out["code"].tolist() == [code], (name, out["code"], code)

    return Job(name, family, 0, lambda h: None, run, check, "tests/test_gpu_parity.py::test_errors_are_loud", refusal=True)


def _one_lag():
    return _lib.LagSet([0.0, 2.0], [0.0], None, None, None)


def _refuse_helio_header(h):
    hs = _sc_h2()[1]
    h.sweep_helioprojective(hs, dict(hs, CDELT1=0.0), _one_lag())


def _refuse_carr_header(h):
    hs = _sc_a()[1]
    h.sweep_carrington(dict(hs, DSUN_OBS=0.0), _lib.Grid(H.CARR_LON, H.CARR_LAT, (32, 32)), SOLAR_R, _one_lag())


def _refuse_order(h):
    hs = _sc_h2()[1]
    h.sweep_helioprojective(hs, hs, _one_lag(), order=7)


def _refuse_mi_helio(h):
    hs = _sc_h2()[1]
    h.sweep_helioprojective(hs, hs, _one_lag(), method=MI)


def _refuse_bins(h):
    h.sweep_set_bins([2.0, 1.0], np.arange(1.0, 9.0))


def _refuse_finalize(h):
    # (a grid-shared sweep stays pending until the next sweep begins: an unsharded sweep first, as
    # test_point_sharded_sweeps_add_up_to_the_unsharded_map does)
    small, hs, large, hl = _sc_b()
    H.gpu_helio(h, small, hs, large, hl, ([0.0], [2.0], None, None, None))
    h.finalize_sums(np.zeros(6), 1)


def _refuse_planes(h):
    from tests import despike_planes_oracle as PO
    h.despike_sum_planes(PO.be(_stack(3, (9, 11), 51, True)), np.zeros(4097, dtype=np.int64), PLANES_RULE)


def _refuse_option(h):
    h.set_option("no_such_option", 1)


# ---- option excursions ----------------------------------------------------------------------------------------------------------
# (option, the value the suite sets it to, its default)
CARR_OPTIONS = [("use_lds", 0, 1), ("pitch", 0, -1), ("tile_w", 8, 0), ("n_groups", 8, 0), ("patch_w", 5, 0),
                ("lds_bytes", 4096, 159 * 1024), ("refine", 0, 1), ("refine_cond_log10", -1, 5), ("tile_skip", 0, 1),
                ("clean_path", 0, 1), ("crop_reference", 0, 1), ("sweep_wgs", 8, 0), ("overlap_upload", 0, 1),
                ("async_upload", 1, 0)]
HELIO_OPTIONS = [("tap_fix", 0, 1), ("border_fix", 0, 1), ("tap_nan_filter", 0, 2), ("h_series", 0, 1), ("h_incr", 0, 1)]
OFF_THE_ORACLE = ("tap_fix", "border_fix")  # (what these two switch off is what makes the zero lag the oracle's)


def carr_options_job():
    shape, lags = (30, 24), lags2(4, 4)
    grid, ls = _lib.Grid(H.CARR_LON, H.CARR_LAT, shape), _lib.LagSet(*lags)
    es_el = lambda: _mi_edges("mi_8x8_5x5")  # noqa: E731  (any valid lists: the chunked sum is compared with itself)

    def one(h, method=CORR):
        small, hs, large, hl = _sc_b()
        h.set_small(small)
        h.prepare_reference_carrington(large, hl, grid, SOLAR_R, 2)
        out = h.sweep_carrington(hs, grid, SOLAR_R, ls, method=method)
        h.drop_small_keepalive()
        return out

    def setup(h):
        h.set_point_shard(0, 1)
        h.set_rotation("reference", None)
        h.set_rotation("small", None)
        h.set_reference_smoothing(None)
        h.set_reference_despike(None)
        h.sweep_set_bins(*es_el())

    def run(h):
        out = {}
        for opt, value, default in CARR_OPTIONS + [("mi_chunks", 2, 0)]:
            h.set_option(opt, value)
            try:
                out[opt] = one(h, MI if opt == "mi_chunks" else CORR)
                out[opt + "_counts"] = h.last_counts()
            finally:
                h.set_option(opt, default)
        return out

    def check(out):
        small, hs, large, hl = _sc_b()
        want = H.oracle_carrington(small, hs, large, hl, lags, shape)
        for opt, _, _ in CARR_OPTIONS:
            H.assert_corr_close(out[opt].reshape(want.shape), want, 1e-10, f"carrington, option {opt}")
        assert np.isfinite(out["mi_chunks"]).all()

    return Job("options_carrington", "carrington", shape[0] * shape[1] * ls.size * len(CARR_OPTIONS), setup, run, check,
               "tests/test_gpu_parity.py::test_sweep_carrington_slices_tiles_groups, ::test_sweep_carrington_vs_oracle (1e-10)")


def helio_options_job():
    lags = ZERO_LAGS

    def setup(h):
        h.set_point_shard(0, 1)
        h.set_reference_smoothing(None)
        h.set_reference_despike(None)

    def run(h):
        out = {}
        for opt, value, default in HELIO_OPTIONS:
            order = 2 if opt == "h_incr" else 1
            small, hs, large, hl = _sc_h1()
            h.set_option(opt, value)
            try:
                out[opt] = H.gpu_helio(h, small, hs, large, hl, lags, order=order)
                out[opt + "_counts"] = h.last_counts()
            finally:
                h.set_option(opt, default)
        return out

    def check(out):
        small, hs, large, hl = _sc_h1()
        for opt, _, _ in HELIO_OPTIONS:
            if opt not in OFF_THE_ORACLE:
                want = H.oracle_helio(small, hs, large, hl, lags, order=2 if opt == "h_incr" else 1)
                H.assert_corr_close(out[opt], want, 1e-7, f"helioprojective, option {opt}")

    return Job("options_helioprojective", "helioprojective", 50 * 50 * 24 * len(HELIO_OPTIONS), setup, run, check,
               "tests/test_gpu_parity.py::test_zero_lag_border_pixels_follow_wcslib, "
               "::test_homography_sweeps_advanced_along_runs_equal_the_per_sample_map (1e-7)")


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
def build():
    order3 = "tests/test_gpu_parity.py::test_other_spline_orders_vs_oracle (1e-7)"
    zero = "tests/test_gpu_parity.py::test_zero_lag_border_pixels_follow_wcslib (1e-7)"
    smooth = "tests/test_gpu_smooth.py::test_carrington_map_of_device_smoothed_images (1e-10)"
    desp = "tests/test_gpu_despike.py::test_carrington_map_of_device_despiked_images (1e-10)"
    ref_shape, ref_lags = (24, 32), lags2(3, 3)
    sm_shape, sm_lags = (30, 22), lags2(4, 3)
    jobs = [
        # 1. Carrington, order 2
        carr_job("carr_f32_g32", _sc_a, (32, 32), lags2(5, 5)),
        carr_job("carr_g20x28_s64", _sc_a, (20, 28), lags2(4, 5)),
        carr_job("carr_g20x28_s40x56", _sc_b, (20, 28), lags2(3, 4)),
        carr_job("carr_f64", _sc_f64, (24, 30), lags2(5, 3),
                 cites="tests/test_gpu_parity.py::test_sweep_carrington_float64_small_image (1e-10)"),
        # 9. the re-evaluation of ill-conditioned lag-points between two scenes with nothing flagged
        _refine_job(),
        # 2. both rotations, then none
        rot_job(),
        carr_job("carr_rot_none", _sc_a, (28, 24), lags2(3, 4), expect_refined=False),
        # 3. the reference image smoothed, despiked, both, neither
        carr_job("ref_smooth", _sc_spiked, ref_shape, ref_lags, smooth=REF_TABLES,
                 oracle_images=lambda: _ref_images(True, False), cites=smooth),
        carr_job("ref_despike", _sc_spiked, ref_shape, ref_lags, despike=REF_RULE,
                 oracle_images=lambda: _ref_images(False, True), cites=desp),
        carr_job("ref_both", _sc_spiked, ref_shape, ref_lags, smooth=REF_TABLES, despike=REF_RULE,
                 oracle_images=lambda: _ref_images(True, True), cites=smooth + ", " + desp),
        carr_job("ref_neither", _sc_spiked, ref_shape, ref_lags, oracle_images=lambda: _ref_images(False, False)),
        # 4. the image to align thresholded, despiked and smoothed, then as it is
        carr_job("small_ops", _sc_spiked, sm_shape, sm_lags, small_ops=(VMAX, SMALL_RULE, SMALL_TABLES),
                 oracle_images=lambda: _small_images(True),
                 cites="tests/test_gpu_smooth.py::test_smoothing_follows_the_threshold, " + desp),
        carr_job("small_plain", _sc_spiked, sm_shape, sm_lags, oracle_images=lambda: _small_images(False)),
        # 5. helioprojective
        helio_job("helio_o1_zero", _sc_h1, 50 * 50, ZERO_LAGS, order=1, cites=zero),
        helio_job("helio_o3_zero", _sc_h3, 44 * 36, ZERO_LAGS, order=3, cites=zero + ", " + order3),
        helio_job("helio_o2_h_incr", _sc_h2, 64 * 64, lags2(4, 3, crota=[0.0, 0.3]), options=(("h_incr", 1, 1),),
                  cites="tests/test_gpu_parity.py::test_homography_sweeps_advanced_along_runs_equal_the_per_sample_map (1e-7)"),
        helio_job("helio_serial", _sc_h2, 64 * 64, lags2(5, 5), serial="f64",
                  cites="tests/test_gpu_parity.py::test_sweep_helioprojective_serial_semantics (1e-7)"),
        helio_job("helio_5d_combo", _sc_h3, 44 * 36, LAGS_5D, combo=(2, 6),
                  cites="tests/test_gpu_parity.py::test_sweep_helioprojective_cdelt_semantics (1e-7)"),
        helio_job("helio_5d_whole", _sc_h3, 44 * 36, LAGS_5D,
                  cites="tests/test_gpu_parity.py::test_sweep_helioprojective_cdelt_semantics (1e-7)"),
        # 6. both wcslib caches evicted inside one launch
        helio_job("helio_70_cdelt1", _sc_48, 48 * 48, LAGS_70, order=1, cites=zero),
        helio_job("helio_70_cdelt1_in_56", _sc_48_in_56, 56 * 56, LAGS_70_REVERSED, order=1, serial="f64", cites=zero),
        # 7. plate carree
        helio_job("car_smallest", _sc_car, 60 * 70, CAR_LAGS, serial="f32", unit="deg",
                  cites="tests/test_gpu_car.py::test_sweep_car_vs_oracle (1e-7)"),
        # 8. the other scores
        residus_job(),
        masked_job(),
        mi_job("mi_8x8_5x5"),
        mi_job("mi_4x12_3x3"),
        # 10. grid shares on one GPU, then an unsharded sweep
        carr_job("carr_two_shares", _sc_b, (26, 22), lags2(3, 3, crota=[0.0, 0.3]), shard=2,
                 cites="tests/test_gpu_parity.py::test_point_sharded_sweeps_add_up_to_the_unsharded_map (1e-10 to the oracle)"),
        carr_job("carr_after_shares", _sc_b, (26, 22), lags2(3, 3, crota=[0.0, 0.3])),
        # 11. iterative context
        context_job("context_2_frames", 0),
        context_job("context_3_frames", 1),
        # 12. pixel-lag sweeps
        pixels_job("pix_sweep", "mi_scene"),
        pixels_job("pix_shifted", "mi_scene", shift=(0.4, -0.3)),
        pixels_job("pix_masked", "mi_scene", method="residus_masked"),
        pixels_job("pix_tiles", "drift", mode="tiles", tile=(16, 20),
                   cites="tests/test_gpu_pxlshift_tiles.py::test_against_the_oracle (equal counts, 2^-23 |corr| + 1e-12)"),
        pixels_job("pix_windows", "drift", mode="windows", tile=(16, 20), step=(7, 9),
                   cites="tests/test_gpu_pxlshift_windows.py::test_stepped_windows_against_the_oracle "
                         "(equal counts, 2^-23 |corr| + 1e-12)"),
        pixels_job("pix_mi", "mi_scene_b", method="mutual_information", bins=8,
                   cites="tests/test_gpu_pxlshift_mi.py::test_against_the_oracle (equal counts, 1e-11)"),
        pixels_job("pix_mi_other_bins", "mi_scene", method="mutual_information", bins=5,
                   cites="tests/test_gpu_pxlshift_mi.py::test_against_the_oracle (equal counts, 1e-11)"),
        destretch_job(),
        # 13. despiked plane sums: "a call leaves the resident images and the reference despiking as they were"
        planes_job("planes_6x40x24", 6, (40, 24), 3, True),
        planes_job("planes_3x16x12", 3, (16, 12), 8, False),
        carr_job("carr_after_planes", _sc_a, (32, 32), lags2(5, 5)),
        # 14. refused calls
        refusal_job("refuse_helio_header", "helioprojective", _refuse_helio_header, _lib.COREG_EINVAL),
        refusal_job("refuse_carrington_header", "carrington", _refuse_carr_header, _lib.COREG_EINVAL),
        refusal_job("refuse_order_7", "helioprojective", _refuse_order, _lib.COREG_EINVAL),
        refusal_job("refuse_mi_on_helioprojective", "helioprojective", _refuse_mi_helio, _lib.COREG_ENOTIMPL),
        refusal_job("refuse_edge_lists", "carrington", _refuse_bins, _lib.COREG_EINVAL),
        refusal_job("refuse_finalize_nothing_pending", "carrington", _refuse_finalize, _lib.COREG_ESTATE),
        refusal_job("refuse_planes_geometry", "planes", _refuse_planes, _lib.COREG_EINVAL),
        refusal_job("refuse_unknown_option", "carrington", _refuse_option, _lib.COREG_EINVAL),
        # 15. option excursions; the jobs that follow run under defaults
        carr_options_job(),
        helio_options_job(),
        carr_job("carr_after_options", _sc_f64, (24, 30), lags2(5, 3)),
    ]
    assert len({j.name for j in jobs}) == len(jobs)
    return jobs


JOBS = build()
BY_NAME = {j.name: j for j in JOBS}
NAMES = [j.name for j in JOBS]

# (a job that leaves a sticky setting, the job that needs it cleared)
TWINS = [("carr_rot_both", "carr_rot_none"), ("ref_smooth", "ref_neither"), ("ref_despike", "ref_neither"),
         ("ref_both", "ref_neither"), ("small_ops", "small_plain"), ("helio_5d_combo", "helio_5d_whole"),
         ("carr_two_shares", "carr_after_shares"), ("pix_shifted", "pix_sweep"), ("mi_8x8_5x5", "mi_4x12_3x3"),
         ("pix_mi", "pix_mi_other_bins"), ("options_carrington", "carr_after_options"),
         ("options_helioprojective", "helio_o1_zero"), ("helio_70_cdelt1", "helio_70_cdelt1_in_56")]
# the sweep a refused call is put in front of
AFTER_REFUSAL = {"helioprojective": "helio_o2_h_incr", "carrington": "carr_g20x28_s40x56", "planes": "planes_3x16x12"}
SEEDS = (20220317, 7, 1143)


def orders():
    """{name: [job names]} -- a job may occur more than once in an order."""
    by_size = sorted(NAMES, key=lambda n: (-BY_NAME[n].size, n))
    twins = []
    for sticky, none in TWINS:
        twins += [sticky, none, sticky]
    refusals = []
    for j in JOBS:
        if j.refusal:
            refusals += [j.name, AFTER_REFUSAL[j.family]]
    out = {"catalogue": list(NAMES), "reversed": NAMES[::-1], "sizes_down_then_up": by_size + by_size[::-1][1:],
           "twins": twins + [none for _, none in TWINS[::-1]], "refusals": refusals}
    for seed in SEEDS:
        out[f"random_{seed}"] = [NAMES[k] for k in np.random.default_rng(seed).permutation(len(NAMES))]
    return out
