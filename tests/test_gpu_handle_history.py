"""
A handle with a past computes what a fresh handle computes, bit for bit.

Every public class runs on a process-wide, long-lived handle (`_lib.shared_handle`), which keeps sticky settings (the two
rotations, the reference smoothing and despiking, two sets of mutual-information edge lists, the pixel-lag sweep's
images and shift, the context frames), caches (the Carrington tables, PlanMemo, the two wcslib caches, the Python-side
`reference_tag`), work space that only grows and one-shot state (the combination range, the grid-shared sums).  The
suite holds each feature to the oracle on the session's handle in one fixed order; this file runs the jobs of
tests/history_jobs.py

  (a) on two fresh handles each: the same bits (the design adds slab sums, refine chunks and tap lists in a fixed order);
  (b) against the oracle of each path, at the tolerance of the existing test the job cites;
  (c) all on ONE handle, in eight orders, each job against its fresh result, bit for bit;
  (d) as public objects on the shared handle, file-backed so that `reference_tag` is live, against a run directly after
      `_lib._close_shared()`.

Two host-side edits, made one at a time in a scratch copy, show that (c) and (d) can fail.  Without `env.sW` / `env.sH`
in `wcslib_cache_key` (sweep_plan.hpp) every order of (c) that holds both `helio_70_cdelt1` and `helio_70_cdelt1_in_56`
goes red (seven of the eight, and the test of the history without edge lists): the second of the two has 2180 samples
where a fresh handle has 2201, the 21 pixels of row 47 that the other job's image drops.  Without
`self.reference_tag = None` in `CoregHandle.set_reference_on_grid` the catalogue order of (d) and the test that counts
preparations go red at the Carrington object that follows the helioprojective one with parallelism=False ("reference-
on-grid shape differs from the Carrington grid").
"""
import os
import warnings

import numpy as np
import pytest

from euispice_coreg_amd import _lib
from tests import helpers as H
from tests import history_jobs as J

pytestmark = pytest.mark.gpu


def first_difference(got, want):
    """None when the two results hold the same arrays bit for bit (NaN equal to NaN), else a description of the first
    entry that differs."""
    if sorted(got) != sorted(want):
        return f"outputs {sorted(got)} / {sorted(want)}"
    for key in sorted(want):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{key}: {a.dtype}{a.shape} / {b.dtype}{b.shape}"
        if not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            same = (a == b) | ((a != a) & (b != b))
            at = np.unravel_index(int(np.argmin(same)), a.shape) if a.ndim else ()
            with np.errstate(invalid="ignore"):
                worst = np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))
            return (f"{key}{list(at)}: {a[at]!r} on this handle, {b[at]!r} on a fresh one "
                    f"({int((~same).sum())} of {a.size} entries differ, largest difference {worst:.3e})")
    return None


def on_a_fresh_handle(job):
    with _lib.CoregHandle(0) as h:
        return job(h)


@pytest.fixture(scope="module")
def fresh():
    """Every job of the catalogue on a fresh handle of its own (one handle open at a time), computed once and left
    unchanged."""
    return {job.name: on_a_fresh_handle(job) for job in J.JOBS}


# ---- (a) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.NAMES)
def test_fresh_runs_repeat(fresh, name):
    again = on_a_fresh_handle(J.BY_NAME[name])
    assert first_difference(again, fresh[name]) is None, f"{name} does not repeat: {first_difference(again, fresh[name])}"


# ---- (b) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.NAMES)
def test_fresh_runs_are_right(fresh, name):
    job = J.BY_NAME[name]
    assert "::" in job.cites  # (the existing test whose tolerance this is)
    job.check(fresh[name])


def test_the_sweep_of_70_cdelt1_lags_needs_both_passes(fresh):
    """Job 6 is not vacuous: each of its 70 lag-points leaves the rows of the image invariant, their border pixels and the
    taps of the order-1 spline are decided by the host's wcslib passes (70 keys: both caches are evicted inside the one
    launch) -- and with the two passes off at least one lag-point differs, as
    tests/test_gpu_parity.py::test_zero_lag_border_pixels_follow_wcslib shows for its scenes."""
    job = J.BY_NAME["helio_70_cdelt1"]
    assert fresh[job.name]["map"].size == 70 and len(np.unique(J.CDELT1_70)) == 70 and 0.0 in J.CDELT1_70
    with _lib.CoregHandle(0) as h:
        h.set_option("border_fix", 0)
        h.set_option("tap_fix", 0)
        raw = job(h)
    d = np.abs(raw["map"] - fresh[job.name]["map"])
    print("lag-points that differ without the passes:", int((d > 0).sum()), "largest", float(np.nanmax(d)))
    assert np.nanmax(d) > 1e-6


# ---- (c) -----------------------------------------------------------------------------------------------------------------
def run_in_order(h, names, fresh):
    """[(position, job name, what differs)] of the jobs of `names`, run one after another on `h`."""
    failures = []
    for k, name in enumerate(names):
        try:
            diff = first_difference(J.BY_NAME[name](h), fresh[name])
        except _lib.CoregError as e:
            diff = f"refused with code {e.code}: {e}"
        if diff is not None:
            failures.append((k, name, diff))
    return failures


def report(order, names, failures):
    lines = [f"order {order!r}: {len(failures)} of {len(names)} jobs differ from their fresh result", "  " + " ".join(names)]
    for k, name, diff in failures:
        lines.append(f"  #{k} {name} after {names[max(0, k - 2):k]}: {diff}")
    return "\n".join(lines)


ORDERS = J.orders()


@pytest.mark.parametrize("order", list(ORDERS))
def test_history_does_not_matter(fresh, order):
    names = ORDERS[order]
    if order in ("catalogue", "reversed", "sizes_down_then_up") or order.startswith("random"):
        assert set(names) == set(J.NAMES)  # (no job dropped)
    with _lib.CoregHandle(0) as h:
        failures = run_in_order(h, names, fresh)
    assert not failures, report(order, names, failures)


def test_mutual_information_without_edge_lists_is_refused_after_any_history_without_them(fresh):
    """The edge lists of `coreg_sweep_set_bins` cannot be taken back, so "MI without bins" is no job of the catalogue: it is
    refused (COREG_ESTATE, check_sweep_mi: before any launch) on a handle whose past holds every job that sets none --
    the pixel-lag sweep's lists included, they are another state -- and the Carrington sweep after it has its bits."""
    names = [n for n in J.NAMES if not n.startswith(("mi_", "options_carrington"))]
    job = J.BY_NAME["carr_g20x28_s40x56"]
    small, hs, large, hl = J._sc_b()
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (20, 28))
    with _lib.CoregHandle(0) as h:
        failures = run_in_order(h, names, fresh)
        assert not failures, report("no edge lists", names, failures)
        job.setup(h)
        with pytest.raises(_lib.CoregError) as e:
            h.sweep_carrington(hs, grid, J.SOLAR_R, _lib.LagSet(*J.lags2(3, 4)), method=J.MI)
        assert e.value.code == _lib.COREG_ESTATE
        assert first_difference(job.run(h), fresh[job.name]) is None


# ---- (d) the classes on the shared handle ---------------------------------------------------------------------------------
LON, LAT, SHAPE = H.CARR_LON, H.CARR_LAT, (32, 28)
LAG1, LAG2 = 17.0 + 2.0 * (np.arange(3) - 1), -9.0 + 2.0 * (np.arange(4) - 1.5)
T_ORIGINAL, T_REWRITTEN = 1_650_000_000_000_000_000, 1_650_000_100_000_000_000
CLASS_RULE = dict(radius=2, n_iter=2, nsigma=5.0, floor=0.0, min_neighbours=5, sign="positive", replace="median")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files the objects read: a 64 x 64 image to align, its 96 x 96 reference image, a second reference image of the
    same size (the pixels a rewritten file gets), a SPICE-like cube with hits in single planes, a pixel-lag pair and the two differential-rotation
    cases of tests/golden/diffrot_alignment_golden."""
    import json
    from euispice_coreg_amd.utils import fits_io
    from tests.conftest import GOLDEN
    from tests.test_despike_planes_cpu import hit_cube
    from tests.pxlshift_tiles_cases import HDR, two_drift_scene
    d = tmp_path_factory.mktemp("history")
    small, hs, large, hl = J.scene((64, 64), 96)
    other = J.with_spikes(J.scene((64, 64), 96, seed=12)[2], 3)
    assert other.shape == large.shape
    out = dict(dir=d, small=str(d / "small.fits"), large=str(d / "large.fits"), rewritten=str(d / "rewritten.fits"),
               hl=hl, pixels=(large.astype(np.float32), other.astype(np.float32)))
    fits_io.write_images(out["small"], [(None, {}), (small.astype(np.float32), hs)])
    fits_io.write_images(out["large"], [(None, {}), (large.astype(np.float32), hl)])
    planes, _, h4, slarge, shl = hit_cube()
    out["spice"] = (planes[None], h4, str(d / "spice_large.fits"))
    fits_io.write_images(out["spice"][2], [(None, {}), (slarge.astype(np.float32), shl)])
    pl, ps, _, _, _ = two_drift_scene()
    out["pxl"] = (str(d / "pxl_large.fits"), str(d / "pxl_small.fits"))
    fits_io.write_images(out["pxl"][0], [(pl, dict(HDR))])
    fits_io.write_images(out["pxl"][1], [(ps, dict(HDR))])
    g = np.load(os.path.join(GOLDEN, "diffrot_alignment_golden.npz"))
    with open(os.path.join(GOLDEN, "diffrot_alignment_golden.json")) as f:
        m = json.load(f)
    out["diffrot"] = {}
    for name in ("b304_given_date", "b174_parallel_order1"):
        c = m["cases"][name]
        p_s, p_l = str(d / f"{name}_small.fits"), str(d / f"{name}_large.fits")
        fits_io.write_images(p_s, [(None, {}), (g["small"], c["hdr_small"])])
        fits_io.write_images(p_l, [(None, {}), (g["large"], c["hdr_large"])])
        out["diffrot"][name] = ((p_s, p_l), c["call"])
    return out


def rewrite(files, which):
    """The reference file of the two `rewritten_*` objects with its first or its second set of pixels -- same path, same
    size, and a modification time of its own."""
    from euispice_coreg_amd.utils import fits_io
    fits_io.write_images(files["rewritten"], [(None, {}), (files["pixels"][which], files["hl"])])
    t = (T_ORIGINAL, T_REWRITTEN)[which]
    os.utime(files["rewritten"], ns=(t, t))


def quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def carrington(files, large=None, order=2, lon=LON, lat=LAT, shape=SHAPE, **kw):
    from euispice_coreg_amd.hdrshift import Alignment
    A = Alignment(files["large"] if large is None else large, files["small"], LAG1, LAG2, None, None, None,
                  reprojection_order=order, **kw)
    corr = quiet(A.align_using_carrington, lonlims=lon, latlims=lat, shape=shape, return_type="corr")
    return dict(corr=np.asarray(corr), counts=np.asarray(A.last_counts))


def helioprojective(files, parallelism, **kw):
    from euispice_coreg_amd.hdrshift import Alignment
    A = Alignment(files["large"], files["small"], LAG1, LAG2, None, None, [0.0, 0.3], parallelism=parallelism)
    corr = quiet(A.align_using_helioprojective, return_type="corr", **kw)
    return dict(corr=np.asarray(corr), counts=np.asarray(A.last_counts))


def diffrot(files, name, reference_date="as the case has it"):
    from tests.test_gpu_diffrot import _align
    paths, call = files["diffrot"][name]
    if reference_date != "as the case has it":
        call = dict(call, reference_date=reference_date)
    return dict(corr=_align(paths, call, "intended"))


def spice(files, **kw):
    """`AlignmentSpice` on the cube of tests/test_despike_planes_cpu.py (60 hits in single wavelength planes), the planes of
    tests/test_gpu_despike_planes.py's interval summed."""
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    cube, h4, p_large = files["spice"]
    S = AlignmentSpice(p_large, (cube, h4), lag_crval1=np.array([-27.0, -23.0, -19.0]), lag_crval2=np.array([32.0, 36.0, 40.0]),
                       parallelism=True, level=2, wavelength_interval_to_sum=[976.74, 977.22], **kw)
    corr = quiet(S.align_using_carrington, lonlims=(242.5, 245.5), latlims=(5.0, 7.5), shape=(30, 40), return_type="corr")
    return dict(corr=np.asarray(corr), counts=np.asarray(S.last_counts), small=np.asarray(S.data_small))


def context(files):
    from tests.test_gpu_iterative_context import run
    from tests.test_iterative_context_cpu import cases, load, scene
    case = load()[1]["cases"][cases()[0]]
    d = files["dir"] / "context"
    if not d.exists():
        d.mkdir()
        files["context"] = scene(case["window"], d)[:2]
    A, res = run(case, *files["context"])
    return dict(corr=np.asarray(res.corr), counts=np.asarray(A.last_counts))


def pixels(files, local=False):
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    A = AlignmentPixels(files["pxl"][0], 0, files["pxl"][1], 0)
    kw = dict(lag_dx=np.arange(-3, 4), lag_dy=np.arange(-2, 3), lag_drot=np.array([0.0]))
    if local:
        F = A.find_local_shifts(**kw, tile_shape=(16, 20), sub_lag=False, min_fill=0.0)
        return dict(corr=np.asarray(F.corr), counts=np.asarray(F.n_samples))
    return dict(corr=A.find_best_parameters(**kw), counts=np.asarray(A.last_counts))


def rewritten(files, which):
    rewrite(files, which)
    return carrington(files, large=files["rewritten"])


# name -> the object's run; the Carrington objects that read `large.fits` name what the tag names
OBJECTS = {
    "carrington": lambda f: carrington(f),
    # (the serial sweep puts the reference image itself on the grid, in place of the Carrington one ...)
    "helioprojective_serial": lambda f: helioprojective(f, False),
    "carrington_again": lambda f: carrington(f),  # (... whose tag must not have survived it)
    "carrington_smooth_large": lambda f: carrington(f, smooth_large=2.0),
    "carrington_despike_large": lambda f: carrington(f, despike_large=J.REF_RULE),
    "diffrot_given_date": lambda f: diffrot(f, "b304_given_date"),
    "diffrot_default_date": lambda f: diffrot(f, "b304_given_date", reference_date=None),
    "diffrot_parallel_order_1": lambda f: diffrot(f, "b174_parallel_order1"),
    "carrington_order_1": lambda f: carrington(f, order=1),
    "carrington_other_grid": lambda f: carrington(f, lon=(232.0, 258.0), lat=(-8.0, 18.0), shape=(24, 30)),
    "rewritten_original": lambda f: rewritten(f, 0),
    "rewritten_other_pixels": lambda f: rewritten(f, 1),
    "helioprojective_parallel": lambda f: helioprojective(f, True),
    # (`fov_limits` is an argument of the helioprojective call alone; it re-grids the image to align on the handle)
    "helioprojective_fov_limits": lambda f: helioprojective(f, True, fov_limits=([-600.0, -50.0], [180.0, 680.0])),
    "spice": lambda f: spice(f),
    "spice_despike_planes": lambda f: spice(f, despike_planes=CLASS_RULE),
    "context": context,
    "pixels": lambda f: pixels(f),
    "local_shifts": lambda f: pixels(f, local=True),
}
OBJECT_SEEDS = (5, 80246)


@pytest.fixture(scope="module")
def expected(files):
    """Every object directly after `_lib._close_shared()`: on a shared handle without a past."""
    out = {}
    for name, run in OBJECTS.items():
        _lib._close_shared()
        out[name] = run(files)
    _lib._close_shared()
    return out


def object_orders():
    names = list(OBJECTS)
    out = {"catalogue": names}
    for seed in OBJECT_SEEDS:
        out[f"random_{seed}"] = [names[k] for k in np.random.default_rng(seed).permutation(len(names))]
    return out


@pytest.mark.parametrize("order", list(object_orders()))
def test_objects_back_to_back_on_the_shared_handle(files, expected, order):
    names = object_orders()[order]
    _lib._close_shared()
    failures = []
    try:
        for k, name in enumerate(names):
            try:
                diff = first_difference(OBJECTS[name](files), expected[name])
            except (_lib.CoregError, ValueError) as e:
                diff = f"raised {type(e).__name__}: {e}"
            if diff is not None:
                failures.append((k, name, diff))
    finally:
        _lib._close_shared()
    assert not failures, report(order, names, failures)


def test_the_objects_are_not_all_the_same(expected):
    """The variants of the Carrington object do change the map: a reference left over from another one would show."""
    base = expected["carrington"]["corr"]
    assert np.array_equal(expected["carrington_again"]["corr"], base, equal_nan=True) and np.isfinite(base).all()
    for name in ("carrington_smooth_large", "carrington_despike_large", "carrington_order_1", "rewritten_other_pixels"):
        assert not np.array_equal(expected[name]["corr"], base, equal_nan=True), name
    assert np.array_equal(expected["rewritten_original"]["corr"], base, equal_nan=True)  # (the same pixels, another path)
    assert not np.array_equal(expected["diffrot_given_date"]["corr"], expected["diffrot_default_date"]["corr"], equal_nan=True)
    assert not np.array_equal(expected["spice"]["small"], expected["spice_despike_planes"]["small"], equal_nan=True)


def test_a_resident_reference_is_reused_only_by_the_object_that_prepared_it(files, monkeypatch):
    """Two consecutive identical Carrington objects: the second skips its preparation (counted as
    tests/test_gpu_jitter.py::test_reference_stays_resident_within_a_sublist counts).  An object that differs in any input
    the tag names -- smoothing, despiking, reference date, order, grid, the file's modification time -- prepares, and so
    does the first object again after each of them."""
    calls = []
    orig = _lib.CoregHandle.prepare_reference_carrington

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(_lib.CoregHandle, "prepare_reference_carrington", spy)

    def prepared(name):
        del calls[:]
        OBJECTS[name](files)
        return len(calls)
    _lib._close_shared()
    try:
        assert prepared("carrington") == 1
        assert prepared("carrington") == 0
        for other in ("carrington_smooth_large", "carrington_despike_large", "carrington_order_1", "carrington_other_grid",
                      "helioprojective_serial", "helioprojective_parallel", "context", "spice"):
            n = prepared(other)
            assert n == (1 if other.startswith(("carrington", "spice")) else 0), other
            assert prepared("carrington") == 1, f"after {other}"
        assert prepared("diffrot_given_date") == 1 and prepared("diffrot_given_date") == 0
        assert prepared("diffrot_default_date") == 1 and prepared("diffrot_given_date") == 1
        assert prepared("rewritten_original") == 1
        assert prepared("rewritten_original") == 0  # (written anew with the same pixels, size and modification time)
        assert prepared("rewritten_other_pixels") == 1 and prepared("rewritten_original") == 1
        # the pixel-lag objects and a despiked plane sum leave the resident reference alone
        assert prepared("carrington") == 1
        for other in ("pixels", "local_shifts"):
            assert prepared(other) == 0
            assert prepared("carrington") == 0, f"after {other}"
    finally:
        _lib._close_shared()
