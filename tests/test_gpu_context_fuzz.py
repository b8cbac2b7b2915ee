"""GPU tests of the iterative-context sweep (coreg_sweep_context: k_context_sweep, k_refine_context,
k_finalize_context_residus) against the independent CPU oracle (oracle/context_oracle.py): a seeded fuzz over raster
shapes, headers, the frame of every column, frame x SPICE dtypes (the four kernel instantiations), NaN / zero / negative
pixels, thresholds, methods, spline orders and CDELT semantics; then one test per edge -- the lag batch of one launch,
the re-evaluation of ill-conditioned lag-points, 'residus' at zero samples (here and in the main helioprojective sweep),
the class's default semantics end to end, and the reuse of one handle across sweeps.

Tolerances: correlation |got - want| <= 1e-8; 'residus' |got - want| <= 1e-8 |want| (the one-pass variance
loses about eps * mean^2 / var: up to 3e-9 relative in these scenes); identical NaN patterns; identical
arg-extremum wherever the best two values differ by more than 1e-6."""
import warnings

import numpy as np
import pytest

from oracle import context_oracle as CO
from tests import context_cases as CC

pytestmark = pytest.mark.gpu

CORR_TOL, RES_RTOL = 1e-8, 1e-8
WORST = {"correlation": 0.0, "residus (relative)": 0.0}


@pytest.fixture(scope="module")
def handle():
    """A handle of this module's own: the options some tests change never reach the session's."""
    from euispice_coreg_amd import _lib
    h = _lib.CoregHandle(0)
    yield h
    h.close()
    print("\n[context fuzz] largest errors:", WORST)


def assert_matches(got, want, method, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs\n{got}\n{want}"
    fin = ~np.isnan(want)
    if not fin.any():
        return
    g, w = got[fin], want[fin]
    if method == "residus":
        err = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)))
        WORST["residus (relative)"] = max(WORST["residus (relative)"], err)
        assert err <= RES_RTOL, f"{what}: relative error {err:.3e}"
        best = np.argsort(w)
    else:
        err = float(np.max(np.abs(g - w)))
        WORST["correlation"] = max(WORST["correlation"], err)
        assert err <= CORR_TOL, f"{what}: max |d| {err:.3e}"
        best = np.argsort(-w)
    if w.size > 1 and abs(w[best[0]] - w[best[1]]) > 1e-6:
        pick = np.argmin(g) if method == "residus" else np.argmax(g)
        assert pick == best[0], f"{what}: arg-extremum differs"


# ---- the seeded fuzz ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(48))
def test_fuzz_matches_the_oracle(handle, seed):
    case = CC.make_case(seed)
    got = CC.gpu(handle, case)
    want = CC.oracle(case)
    assert_matches(got, want, case["method"], f"seed {seed}")


@pytest.mark.parametrize("fd,sd", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32),
                                   (np.float64, np.float64)])
@pytest.mark.parametrize("method", ["correlation", "residus"])
def test_every_dtype_instantiation(handle, fd, sd, method):
    """Each <frame, SPICE> instantiation on one scene: odd width (a one-column tail group), a new frame every column
    (frames change inside a workgroup's column pair), both thresholds."""
    case = CC.make_case(1000, gW=7, gH=100, method=method, order=2, frame_dtype=fd, spice_dtype=sd, n_frames=3,
                        col_mode="every", thresholds="both", nan_frac=0.0, zeros=False)
    assert_matches(CC.gpu(handle, case), CC.oracle(case), method, f"{fd.__name__} x {sd.__name__}")


# ---- the lag batch of one launch (kCtxBatch = 8192) -----------------------------------------------------------------
def test_batch_boundary(handle):
    c1 = np.linspace(-6.0, 6.0, 97) * CC.AS
    c2 = np.linspace(5.0, -5.0, 91) * CC.AS
    case = CC.make_case(2000, gW=3, gH=7, method="correlation", order=2, semantics=CO.INTENDED, n_frames=2,
                        col_mode="every", thresholds="none", nan_frac=0.0, lags=[c1, c2, None, None, None])
    n = 97 * 91
    assert n > 8192
    whole = CC.gpu(handle, case).ravel()
    parts = [CC.gpu(handle, case, upload_first=False, lag_begin=b, lag_end=e)
             for b, e in ((0, 4000), (4000, 8192), (8192, n))]
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)
    tail = CC.gpu(handle, case, upload_first=False, lag_begin=8000, lag_end=n)
    assert np.array_equal(tail, whole[8000:], equal_nan=True)
    idx = np.sort(np.random.default_rng(5).choice(n, 64, replace=False))
    idx = np.unique(np.concatenate([idx, [0, 8191, 8192, n - 1]]))
    want = CC.oracle(case, lag_index=idx).ravel()[idx]
    assert_matches(whole[idx], want, "correlation", "batch subset")
    assert np.isfinite(want).sum() > 40


# ---- the re-evaluation of ill-conditioned lag-points ------------------------------------------------------------------
def far_pivot_case():
    """Frames that hold a large constant everywhere outside the footprint of the raster at every lag: the pivot of the
    context sums (the mean of all frame pixels) lies far from every lag-point's own mean."""
    lags = [np.array([-4.0, 0.0, 4.0]) * CC.AS, np.array([3.0, -3.0]) * CC.AS, None, None, np.array([0.0, 0.5])]
    case = CC.make_case(3000, gW=6, gH=40, method="correlation", order=2, semantics=CO.INTENDED, n_frames=2,
                        col_mode="blocks", thresholds="none", nan_frac=0.0, frame_dtype=np.float64,
                        spice_dtype=np.float64, lags=lags)
    ny, nx = case["hdr_small"]["NAXIS2"], case["hdr_small"]["NAXIS1"]
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    _, table = CO.lag_table(lags)
    from oracle import coreg_oracle as O
    for f, (img, hf) in enumerate(zip(case["frames"], case["frame_headers"])):
        keep = np.zeros(img.shape, dtype=bool)
        for lag in table:
            ctx, _, _ = CO.lag_headers(case["target4"], case["hdr_small"], *lag)
            ox, oy, _, _ = O.wcslib_pixel_to_pixel(ctx, hf, xx, yy)
            x0, x1 = int(np.floor(ox.min())) - 3, int(np.ceil(ox.max())) + 4
            y0, y1 = int(np.floor(oy.min())) - 3, int(np.ceil(oy.max())) + 4
            keep[max(y0, 0):y1, max(x0, 0):x1] = True
        img[~keep] = 1e6
        assert (~keep).mean() > 0.5
    return case


def test_refinement_of_a_far_pivot(handle):
    case = far_pivot_case()
    got = CC.gpu(handle, case)
    refined = handle.last_visit_counts()["refined_lag_points"]
    assert refined > 0
    want = CC.oracle(case)
    assert np.isfinite(want).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.max(np.abs(got - want)) <= 1e-10, np.max(np.abs(got - want))
    print(f"\n[context fuzz] far pivot: {refined} of {want.size} lag-points refined")
    # "refine" = 0: the one-pass values, nothing counted -- and a sweep after it starts its count from zero
    try:
        handle.set_option("refine", 0)
        CC.gpu(handle, case, upload_first=False)
        assert handle.last_visit_counts()["refined_lag_points"] == 0
    finally:
        handle.set_option("refine", 1)
    CC.gpu(handle, case, upload_first=False)
    assert handle.last_visit_counts()["refined_lag_points"] == refined


@pytest.mark.parametrize("fd,sd", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32),
                                   (np.float64, np.float64)])
def test_refining_every_lag_point_changes_nothing(handle, fd, sd):
    case = CC.make_case(4000, gW=5, gH=60, method="correlation", order=2, semantics=CO.INTENDED, frame_dtype=fd,
                        spice_dtype=sd, n_frames=3, col_mode="every", thresholds="min", nan_frac=0.01)
    default = CC.gpu(handle, case)
    assert np.isfinite(default).sum() >= 4
    try:
        handle.set_option("refine_cond_log10", -1)
        every = CC.gpu(handle, case, upload_first=False)
        refined = handle.last_visit_counts()["refined_lag_points"]
    finally:
        handle.set_option("refine_cond_log10", 5)
    assert refined >= np.isfinite(default).sum()
    assert np.array_equal(np.isnan(every), np.isnan(default))
    assert np.nanmax(np.abs(every - default)) <= 1e-12, np.nanmax(np.abs(every - default))


# ---- 'residus' at zero samples ----------------------------------------------------------------------------------------
def zero_block_case():
    """A 3 x 3 block of exact zeros in the frame under the grid point of the smallest SPICE value: the order-2 context
    sample there is exactly 0, and the SPICE sample is positive.  `vmin` = 1 keeps every finite SPICE sample (all are
    above 100) and drops the NaN ones of the border, so that without the block every lag-point is a number.  Returns the
    case and the largest SPICE sample at a zero context sample over the lags (a `vmin` above it drops them all)."""
    case = CC.make_case(5000, gW=5, gH=24, method="residus", order=2, semantics=CO.INTENDED, n_frames=1,
                        col_mode="one", thresholds="none", nan_frac=0.0, zeros=False, frame_dtype=np.float64,
                        spice_dtype=np.float64, lags=[np.array([-0.5, 0.0, 0.5]) * CC.AS, np.array([0.0]), None, None,
                                                      None])
    case["vmin"] = 1.0
    assert np.nanmin(case["spice"]) > 100.0
    assert np.isfinite(CC.oracle(case)).all()
    args = [case[k] for k in ("frames", "frame_headers", "col_frame", "spice", "target4", "hdr_small")]
    _, a, b = CO.context_step(*args, (0.0, 0.0, 0.0, 0.0, 0.0), method="residus", samples=True)
    nx = case["hdr_small"]["NAXIS1"]
    inner = np.zeros((case["hdr_small"]["NAXIS2"], nx), dtype=bool)
    inner[2:-2, 1:-1] = True
    k = int(np.argmin(np.where(inner.ravel(), b, np.inf)))
    ctx, _, _ = CO.lag_headers(case["target4"], case["hdr_small"], 0.0, 0.0, 0.0, 0.0, 0.0)
    from oracle import coreg_oracle as O
    ox, oy, _, _ = O.wcslib_pixel_to_pixel(ctx, case["frame_headers"][0], [float(k % nx)], [float(k // nx)])
    cx, cy = int(np.rint(ox[0])), int(np.rint(oy[0]))
    case["frames"][0][cy - 1:cy + 2, cx - 1:cx + 2] = 0.0
    bz = []
    for lag in CO.lag_table(case["lags"])[1]:
        _, a, b = CO.context_step(*args, lag, method="residus", samples=True)
        bz.append(b[a == 0.0])
    bz = np.concatenate(bz)
    assert bz.size and (bz > 0).all()
    return case, float(bz.max())


def test_residus_is_nan_at_a_zero_context_sample(handle):
    """np.std over (a - b) / sqrt(a) with a = 0, b > 0 is NaN (an infinite term); the one-pass moments gave
    fmax(inf - inf, 0) = 0.0 there, the best possible score."""
    case, bz = zero_block_case()
    want = CC.oracle(case)
    assert np.isnan(want[1, 0, 0, 0, 0])  # the zero lag samples the block (and nothing else makes it NaN)
    got = CC.gpu(handle, case)
    assert_matches(got, want, "residus", "zero block")
    # a threshold that drops those points: finite, matching
    case["vmin"] = bz * (1 + 1e-6)
    want = CC.oracle(case)
    assert np.isfinite(want).all()
    assert_matches(CC.gpu(handle, case), want, "residus", "zero block, vmin")


def test_helioprojective_residus_is_nan_at_a_zero_reference_sample(gpu_handle):
    """The main helioprojective sweep, the reference image on its own grid (alignment.py's serial branch): a grid inside
    the image to align, so that every grid point overlaps and 'residus' is a number -- until one reference pixel is 0.
    (point_lag drops a non-finite term, so the lag-point lacks a grid point and k_finalize reports NaN.)"""
    from euispice_coreg_amd import _lib, synthetic
    from oracle import coreg_oracle as O
    from tests import helpers as H
    small, hs, _, _, _ = H.scene(small_n=64, large_n=96, nan_frac=0.0)
    hl = synthetic._header(24, 24, 12.5, 12.5, hs["CRVAL1"], hs["CRVAL2"], 20.0, 20.0, 1.0)
    yy, xx = np.mgrid[0:24, 0:24].astype(np.float64)
    ox, oy, _, _ = O.wcslib_pixel_to_pixel(hl, hs, xx, yy)
    large = O.spline_sample_model(small, ox, oy, np.nan, 2).reshape(24, 24) + 10.0
    assert np.isfinite(large).all() and (large > 0).all()
    lags = ([-2.0, 0.0, 2.0], [0.0, 1.0], None, None, None)

    def both(large):
        st = H.oracle_state(small, hs, large, hl, lags)
        want = O.find_best_header_parameters(st, "helioprojective", method="residus", parallelism=False)
        gpu_handle.set_small(small)
        gpu_handle.set_reference_on_grid(np.asarray(large, dtype=np.float64))
        got = gpu_handle.sweep_helioprojective(hl, hs, _lib.LagSet(*lags), method=_lib.METHOD_RESIDUS)
        return got.reshape(want.shape), want

    got, want = both(large)
    assert np.isfinite(want).all()
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-9, np.max(np.abs(got - want) / np.abs(want))
    z = large.copy()
    z[10:13, 11:14] = 0.0
    got, want = both(z)
    assert np.isnan(want).all()
    assert np.isnan(got).all(), got


# ---- the class's default semantics, end to end ------------------------------------------------------------------------
def test_class_default_semantics_match_the_oracle(tmp_path):
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster
    from euispice_coreg_amd.utils import fits_io
    from tests.test_iterative_context_cpu import prepared, scene
    lags = [[-4.0, 0.0, 4.0], [-2.0, 3.0], [0.0, 0.2], [-0.05, 0.0], None]
    (tmp_path / "run").mkdir()
    p_spice, paths, c = scene("P05", tmp_path / "run")
    A = AlignementSpiceIterativeContextRaster(
        large_fov_list_paths=paths, small_fov_to_correct=p_spice, threshold_time=c["threshold_time"],
        lag_crval1=np.array(lags[0]), lag_crval2=np.array(lags[1]), lag_cdelt1=np.array(lags[2]),
        lag_cdelt2=np.array(lags[3]), lag_crota=None, small_fov_window=0)
    assert A.cdelt_semantics == "intended"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = np.asarray(A.align_using_helioprojective(method="correlation").corr)[..., 0]
    # the oracle's inputs: the same scene, prepared as the class prepares it
    (tmp_path / "oracle").mkdir()
    B, target, headers, cf = prepared("P05", tmp_path / "oracle", lags)
    frames = [np.asarray(fits_io.read_image(p, -1)[0]) for p in B.large_fov_list_paths]
    want = CO.context_sweep(frames, headers, cf, np.asarray(B.data_small, dtype=np.float64), target, B.hdr_small,
                            (B.lag_crval1, B.lag_crval2, B.lag_cdelt1, B.lag_cdelt2, B.lag_crota),
                            semantics=CO.INTENDED)
    assert np.isfinite(want).all()  # (CDELT2 lags evaluated: not the reference's dead workers)
    assert_matches(got, want, "correlation", "class default")


# ---- one handle across sweeps ------------------------------------------------------------------------------------------
def test_handle_reuse_across_scenes(handle):
    a = CC.make_case(6000, gW=5, gH=100, method="correlation", order=2, n_frames=3, col_mode="every",
                     thresholds="none", frame_dtype=np.float32, spice_dtype=np.float64)
    b = CC.make_case(6001, gW=12, gH=7, method="correlation", order=4, n_frames=8, col_mode="random",
                     thresholds="min", frame_dtype=np.float64, spice_dtype=np.float32)
    assert np.prod([len(v) for v in a["lags"] if v is not None]) != np.prod([len(v) for v in b["lags"] if v is not None])
    first = CC.gpu(handle, a)
    other = CC.gpu(handle, b)
    again = CC.gpu(handle, a)
    assert np.array_equal(first, again, equal_nan=True)
    assert_matches(first, CC.oracle(a), "correlation", "scene A")
    assert_matches(other, CC.oracle(b), "correlation", "scene B")
