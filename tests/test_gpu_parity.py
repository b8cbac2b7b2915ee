"""
GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI
(euispice_coreg_amd/_lib.py -> libcoreg_hip.so), against the CPU oracle on the same seeded inputs
and against the committed golden vectors produced by the reference's own rectify.py.

Tolerances (float64 arithmetic on both sides; stated per test):
  * resampled images: |d| <= 1e-9 * max|image| (coordinate differences ~1e-12 px from libm vs ocml atan/sin)
  * corr maps: 1e-10 when the latitude trig tables are NumPy's (bit-identical inputs), 1e-6 when the library
    computes correctly-rounded float32 lat trig itself (SURVEY quirk Q6, fp32-trig ambiguity); identical argmax.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests.conftest import rectify_case

pytestmark = pytest.mark.gpu


def _lags(n1=5, n2=5, step=2.0, c1=17.0, c2=-9.0, cdelt1=None, cdelt2=None, crota=None):
    return (c1 + step * (np.arange(n1) - n1 // 2), c2 + step * (np.arange(n2) - n2 // 2), cdelt1, cdelt2, crota)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_resample_carrington_matches_reference_golden(gpu_handle, rectify_golden, case):
    """coreg_resample_carrington == reference rectify.Rectifier(CarringtonTransform) output (golden vectors)."""
    from euispice_coreg_amd import _lib
    c = rectify_case(rectify_golden, case)
    gpu_handle.set_small(c["image"])
    grid = _lib.Grid(c["lonlims"], c["latlims"], c["shape"], numpy_lat_trig=True)
    out = gpu_handle.resample_carrington(c["hdr"], grid, c["solar_r"], order=c["order"])
    want = c["resampled"]
    assert out.shape == want.shape
    # points whose coordinate sits within 1e-9 px of the bounds rule may legitimately flip
    W, Hh = c["image"].shape[1], c["image"].shape[0]
    with np.errstate(invalid="ignore"):
        edge = (np.abs(c["nx"]) < 1e-9) | (np.abs(c["nx"] - (W - 1)) < 1e-9) | (np.abs(c["ny"]) < 1e-9) | \
               (np.abs(c["ny"] - (Hh - 1)) < 1e-9)
    same_nan = np.isnan(out) == np.isnan(want)
    assert (same_nan | edge).all()
    m = np.isfinite(out) & np.isfinite(want)
    assert m.sum() > 100
    assert np.abs(out[m] - want[m]).max() <= 1e-9 * np.nanmax(np.abs(c["image"]))


def test_resample_carrington_library_lat_trig_close(gpu_handle, rectify_golden):
    """With the library's own (correctly rounded) float32 latitude trig the result moves by the fp32-trig
    ambiguity only (quirk Q6): coordinates <= ~1e-3 px -> samples within 1e-3 of the image range."""
    from euispice_coreg_amd import _lib
    c = rectify_case(rectify_golden, "A")
    gpu_handle.set_small(c["image"])
    grid = _lib.Grid(c["lonlims"], c["latlims"], c["shape"], numpy_lat_trig=False)
    out = gpu_handle.resample_carrington(c["hdr"], grid, c["solar_r"], order=c["order"])
    m = np.isfinite(out) & np.isfinite(c["resampled"])
    assert m.sum() > 0.95 * np.isfinite(c["resampled"]).sum()
    assert np.abs(out[m] - c["resampled"][m]).max() <= 1e-3 * np.nanmax(np.abs(c["image"]))


@pytest.mark.parametrize("order", [1, 2])
def test_resample_helioprojective_vs_oracle(gpu_handle, order):
    small, hs, large, hl, _ = H.scene(small_n=80, large_n=128)
    from oracle import coreg_oracle as O
    st = H.oracle_state(small, hs, large, hl, _lags(), order=order)
    O.set_initial_header_values(st)
    sub = O.create_submap_of_large_data(st)  # hdr_large := hdr_small
    hdr_shift = dict(st.hdr_small)
    O.shift_header(st, hdr_shift, 21.0, -5.0, 0.0, 0.0, 0.4)
    want = O.interpolate_on_large_data_grid(st, st.data_small, hdr_shift)
    gpu_handle.set_small(small)
    got = gpu_handle.resample_helioprojective(st.hdr_small, hdr_shift, order=order)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = np.isfinite(want)
    assert m.sum() > 1000
    # float32 outputs: equal up to one float32 ulp where the float64 value sits on a rounding boundary
    assert np.abs(got[m].astype(np.float64) - want[m]).max() <= 2e-7 * np.abs(want[m]).max()
    # the once-only reference preparation
    gpu_handle.prepare_reference_helioprojective(large, hl, hs, order)
    ref = gpu_handle.get_reference_on_grid(sub.shape, np.float32)
    assert np.array_equal(np.isnan(ref), np.isnan(sub))
    m = np.isfinite(sub)
    assert np.abs(ref[m].astype(np.float64) - sub[m]).max() <= 2e-7 * np.abs(sub[m]).max()


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("use_lds", [0, 1])
def test_sweep_carrington_vs_oracle(gpu_handle, order, use_lds):
    small, hs, large, hl, _ = H.scene()
    lags = _lags(7, 6)
    shape = (72, 64)
    want = H.oracle_carrington(small, hs, large, hl, lags, shape, order=order)
    gpu_handle.set_option("use_lds", use_lds)
    try:
        got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, order=order)
    finally:
        gpu_handle.set_option("use_lds", 1)
    H.assert_corr_close(got, want, 1e-10, f"carrington order={order} lds={use_lds}")
    st = gpu_handle.last_stats()
    assert st["n_lags"] == 42 and st["used_lds"] == use_lds
    # reference on the grid itself
    from oracle import coreg_oracle as O
    a = O.carrington_transform_fa(np.asarray(large, float), hl, 1.004, list(shape), list(H.CARR_LON), list(H.CARR_LAT),
                                  order)
    ref = gpu_handle.get_reference_on_grid(a.shape, np.float64)
    m = np.isfinite(a) & np.isfinite(ref)
    assert m.sum() > 0.98 * np.isfinite(a).sum()
    assert np.abs(ref[m] - a[m]).max() <= 1e-9 * np.nanmax(a)


def test_sweep_carrington_library_lat_trig(gpu_handle):
    """Library-computed latitude trig: corr within the stated 1e-6 and same argmax (quirk Q6)."""
    small, hs, large, hl, _ = H.scene()
    lags = _lags(7, 7)
    shape = (72, 64)
    want = H.oracle_carrington(small, hs, large, hl, lags, shape)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, numpy_lat_trig=False)
    H.assert_corr_close(got, want, 1e-6, "carrington, library lat trig")


def test_sweep_carrington_5d_lags(gpu_handle):
    """CROTA and CDELT lags (intended CDELT semantics, quirk Q2) on the Carrington path."""
    small, hs, large, hl, _ = H.scene()
    lags = _lags(4, 3, cdelt1=[-0.05, 0.0, 0.05], cdelt2=[0.0, 0.04], crota=[-0.5, 0.0, 0.3])
    shape = (64, 56)
    want = H.oracle_carrington(small, hs, large, hl, lags, shape)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape)
    assert got.shape == (4, 3, 3, 2, 3, 1)
    H.assert_corr_close(got, want, 1e-10, "carrington 5-D")


def test_sweep_carrington_float64_small_image(gpu_handle):
    """Pixel values that are not float32-exact take the float64 storage path."""
    small, hs, large, hl, _ = H.scene(float32_exact=False)
    lags = _lags(5, 5)
    shape = (64, 64)
    want = H.oracle_carrington(small, hs, large, hl, lags, shape)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape)
    assert gpu_handle.last_stats()["small_is_f32"] == 0
    H.assert_corr_close(got, want, 1e-10, "carrington f64 storage")


def test_sweep_carrington_slices_tiles_groups(gpu_handle):
    """np.array_split-style lag slices concatenate to the full map; tile shape / group count / LDS size do not
    change results beyond summation-order rounding."""
    small, hs, large, hl, _ = H.scene()
    lags = _lags(9, 7, crota=[0.0, 0.25])
    shape = (80, 72)
    full = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape)
    n = full.size
    parts = []
    for lo, hi in [(0, 17), (17, 18), (18, 18), (18, 95), (95, n)]:
        parts.append(H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, lag_begin=lo, lag_end=hi,
                                      prepare=False))
    cat = np.concatenate(parts)
    # culling depends on the slice's lag range, so points are grouped differently: equal up to summation rounding
    assert np.array_equal(np.isnan(cat), np.isnan(full.ravel()))
    assert np.nanmax(np.abs(cat - full.ravel())) <= 1e-12
    for opt, val in [("tile_w", 8), ("tile_w", 128), ("n_groups", 8), ("n_groups", 64), ("lds_bytes", 4096),
                     ("lds_bytes", 64 * 1024), ("patch_w", 5), ("patch_w", 64)]:
        gpu_handle.set_option(opt, val)
        try:
            alt = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, prepare=False)
        finally:
            gpu_handle.set_option("tile_w", 0)
            gpu_handle.set_option("n_groups", 0)
            gpu_handle.set_option("lds_bytes", 159 * 1024)
            gpu_handle.set_option("patch_w", 0)
        assert np.nanmax(np.abs(alt - full)) <= 1e-12, (opt, val)


def test_sweep_no_overlap_is_nan(gpu_handle):
    """A lag that moves the small image completely off the grid -> empty mask -> NaN (the reference's numba
    routine divides by zero there, SURVEY a-15)."""
    small, hs, large, hl, _ = H.scene()
    lags = (np.array([17.0, 40000.0]), np.array([-9.0]), None, None, None)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (64, 64))
    assert np.isfinite(got[0, 0, 0, 0, 0, 0]) and np.isnan(got[1, 0, 0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("use_lds", [0, 1])
def test_sweep_helioprojective_vs_oracle(gpu_handle, order, use_lds):
    small, hs, large, hl, _ = H.scene(small_n=80, large_n=128)
    lags = _lags(6, 5, crota=[0.0, 0.3])
    want = H.oracle_helio(small, hs, large, hl, lags, order=order)
    gpu_handle.set_option("use_lds", use_lds)
    try:
        got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
    finally:
        gpu_handle.set_option("use_lds", 1)
    # float32-rounded samples on both sides: a handful of samples may round differently (1 float32 ulp)
    H.assert_corr_close(got, want, 1e-7, f"helio order={order} lds={use_lds}")


def test_homography_exact_division_path_equals_series_path(gpu_handle):
    """The projective denominator is inverted by the series 1 - eps + eps^2 when the host proves |eps| < 4e-6, by
    v_rcp_f64 + a Newton step otherwise (wide fields of view); both agree with the oracle and with each other."""
    small, hs, large, hl, _ = H.scene(small_n=80, large_n=128)
    lags = _lags(5, 4, crota=[0.0, -0.4])
    want = H.oracle_helio(small, hs, large, hl, lags)
    gpu_handle.set_option("h_series", 0)
    try:
        exact = H.gpu_helio(gpu_handle, small, hs, large, hl, lags)
        assert gpu_handle.last_sweep_variant()["mode"] == 1  # (sweep_variant.hpp kHomography: exact division ran)
    finally:
        gpu_handle.set_option("h_series", 1)
    series = H.gpu_helio(gpu_handle, small, hs, large, hl, lags)
    assert gpu_handle.last_sweep_variant()["mode"] == 2  # (kHomographySeries: the host proved eps_max < 4e-6)
    H.assert_corr_close(exact, want, 1e-7, "helio, exact division")
    H.assert_corr_close(series, want, 1e-7, "helio, series inverse")
    assert np.nanmax(np.abs(exact - series)) <= 1e-9


@pytest.mark.parametrize("series", [1, 0])
@pytest.mark.parametrize("nan_frac", [0.0, 0.01])
def test_homography_sweeps_advanced_along_runs_equal_the_per_sample_map(gpu_handle, series, nan_frac):
    """Round 6 (`h_incr`, kernels.hpp tile_points kIncr): on interior LDS visits of an order-2 homography sweep the affine
    terms of a lane's map are advanced by additions along runs of a grid row, with the window offset folded into the map.
    Same map as the per-sample evaluation to 1e-11, with NaN pixels in the reference image (runs broken by culled points)
    and without (the unmasked CLEAN path), series and exact-division variants; both against the oracle."""
    small, hs, large, hl, _ = H.scene(small_n=160, large_n=200, nan_frac=nan_frac)
    large = large.copy()
    large[60:64, 70:90] = np.nan  # culled grid points: chunks that are not runs
    lags = _lags(5, 4, crota=[0.0, -0.4])
    want = H.oracle_helio(small, hs, large, hl, lags)
    gpu_handle.set_option("h_series", series)
    try:
        maps = []
        for incr in (1, 0):
            gpu_handle.set_option("h_incr", incr)
            maps.append(H.gpu_helio(gpu_handle, small, hs, large, hl, lags))
            assert gpu_handle.last_visit_counts()["interior"] > 0
            # (sweep_variant.hpp: kHomographySeries = 2, kHomography = 1 -- the variant the parameter names did run)
            assert gpu_handle.last_sweep_variant()["mode"] == (2 if series else 1)
    finally:
        gpu_handle.set_option("h_series", 1)
        gpu_handle.set_option("h_incr", 1)
    H.assert_corr_close(maps[0], want, 1e-7, "helio, advanced along runs")
    H.assert_corr_close(maps[1], want, 1e-7, "helio, per-sample map")
    assert np.nanmax(np.abs(maps[0] - maps[1])) <= 1e-11


def test_sweep_helioprojective_serial_semantics(gpu_handle):
    """parallelism=False path of the reference (quirk Q1): target = FULL large-FOV grid, float64 reference."""
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=96)
    lags = _lags(5, 5)
    want = H.oracle_helio(small, hs, large, hl, lags, parallelism=False)
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, serial_semantics=True)
    H.assert_corr_close(got, want, 1e-7, "helio serial semantics")
    st = gpu_handle.last_stats()
    assert st["n_active_points"] < st["n_grid_points"]  # most of the large grid never sees the small image


def test_sweep_helioprojective_spice_like_degrees(gpu_handle):
    """SPICE-like raster: header in degrees, CDELT1 != CDELT2, lags given in arcsec and converted
    (alignment.py:819-837), CROTA lags (config 4 shape, reduced)."""
    small, hs, large, hl, _ = H.scene(small_shape=(104, 48), small_cdelt=(4.0 * 5, 1.098 * 9), small_unit="deg",
                                      large_n=128)
    lags_arcsec = _lags(5, 5, step=8.0, crota=[-0.4, 0.0, 0.4])
    want = H.oracle_helio(small, hs, large, hl, lags_arcsec, unit_lag="arcsec")
    lags_deg = (lags_arcsec[0] / 3600.0, lags_arcsec[1] / 3600.0, None, None, lags_arcsec[4])
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags_deg)
    H.assert_corr_close(got, want, 1e-7, "helio SPICE-like")


def test_sweep_helioprojective_cdelt_semantics(gpu_handle):
    """CDELT lags: intended semantics match the oracle; reference semantics: d_cdelt2 != 0 -> NaN (dead worker),
    d_cdelt1 != 0 only forces the PC rebuild (quirk Q2/Q3)."""
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=96)
    lags = _lags(3, 3, cdelt1=[0.0, 0.05], cdelt2=[0.0, -0.04])
    want = H.oracle_helio(small, hs, large, hl, lags)
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags)
    H.assert_corr_close(got, want, 1e-7, "helio cdelt intended")
    got_ref = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, cdelt_semantics=1)
    assert np.isnan(got_ref[:, :, :, 1]).all() and np.isfinite(got_ref[:, :, :, 0]).all()
    lags1 = _lags(3, 3, cdelt1=[0.0, 0.05])
    want1 = H.oracle_helio(small, hs, large, hl, lags1, cdelt_semantics="reference")
    got1 = H.gpu_helio(gpu_handle, small, hs, large, hl, lags1, cdelt_semantics=1)
    H.assert_corr_close(got1, want1, 1e-7, "helio cdelt1 reference semantics")


def test_method_residus(gpu_handle):
    """method='residus' (alignment.py:544-547): np.std((A - B) / sqrt(A)) over ALL grid pixels, no NaN mask (quirk Q8):
    a number only when every grid pixel overlaps, NaN otherwise."""
    from euispice_coreg_amd import _lib
    from oracle import coreg_oracle as O
    small, hs, large, hl, _ = H.scene(nan_frac=0.0)
    lags = _lags(3, 3)
    # grid well inside the small FOV for every lag: full overlap -> finite
    lon, lat, shape = (243.0, 249.0), (2.0, 8.0), (40, 36)
    st = H.oracle_state(small, hs, large, hl, lags, shape=list(shape), lonlims=list(lon), latlims=list(lat),
                        solar_r=(1.004,))
    want = O.find_best_header_parameters(st, "carrington", method="residus")
    assert np.isfinite(want).all()
    grid = _lib.Grid(lon, lat, shape)
    ls = _lib.LagSet(*lags)
    gpu_handle.set_small(small)
    gpu_handle.prepare_reference_carrington(large, hl, grid, 1.004, 2)
    got = gpu_handle.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_RESIDUS).reshape(want.shape)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert np.argmin(got) == np.argmin(want)
    # the usual grid (partly outside the FOV): NaN for every lag, as in the reference
    st = H.oracle_state(small, hs, large, hl, lags, shape=[48, 40], lonlims=list(H.CARR_LON), latlims=list(H.CARR_LAT),
                        solar_r=(1.004,))
    want = O.find_best_header_parameters(st, "carrington", method="residus")
    assert np.isnan(want).all()
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (48, 40))  # correlation still fine there
    assert np.isfinite(got).all()
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    got = gpu_handle.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_RESIDUS)
    assert np.isnan(got).all()
    # helioprojective: float32 arithmetic in the reference (float32 sub-map and sample) -> 1e-5 relative
    s2, hs2, l2, hl2, _ = H.scene(small_n=64, large_n=96, nan_frac=0.0)
    st = H.oracle_state(s2, hs2, l2, hl2, ([0.0], [0.0], None, None, None))
    want = O.find_best_header_parameters(st, "helioprojective", method="residus")
    gpu_handle.set_small(s2)
    gpu_handle.prepare_reference_helioprojective(l2, hl2, hs2, 2)
    got = gpu_handle.sweep_helioprojective(hs2, hs2, _lib.LagSet([0.0], [0.0], None, None, None),
                                           method=_lib.METHOD_RESIDUS)
    assert np.isnan(want).all() == np.isnan(got).all()
    if np.isfinite(want).all():
        assert abs(got[0] - want.ravel()[0]) <= 1e-5 * abs(want.ravel()[0])


def test_errors_are_loud(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene(small_n=48, large_n=64)
    h2 = _lib.CoregHandle(0)
    try:
        with pytest.raises(_lib.CoregError):  # nothing uploaded yet
            h2.sweep_helioprojective(hs, hs, _lib.LagSet([0.0], [0.0], None, None, None))
        h2.set_small(small)
        h2.prepare_reference_helioprojective(large, hl, hs, 2)
        with pytest.raises(_lib.CoregError):  # spline order outside scipy's 0..5
            h2.sweep_helioprojective(hs, hs, _lib.LagSet([0.0], [0.0], None, None, None), order=7)
        with pytest.raises(_lib.CoregError):  # unknown method: refuse, never fall back
            h2.sweep_helioprojective(hs, hs, _lib.LagSet([0.0], [0.0], None, None, None), method=7)
        with pytest.raises(_lib.CoregError):
            h2.set_option("no_such_option", 1)
    finally:
        h2.close()


@pytest.mark.parametrize("order", [1, 2, 3])
def test_infinite_pixels_are_masked_as_the_reference_masks_them(gpu_handle, order):
    """alignment.py:525 masks with `isfinite`, and a spline tap on a +-Inf pixel gives +-Inf (weight != 0) or NaN
    (weight == 0, or both signs among the taps): an infinite pixel takes out exactly the samples a NaN pixel would, in
    the image to align and in the reference image alike (where it also passes through the once-only resampling)."""
    small, hs, large, hl, truth = H.scene(small_n=96, large_n=160)
    small, large = small.copy(), large.copy()
    rng = np.random.default_rng(17)
    for img, n in ((small, 40), (large, 25)):
        yy, xx = rng.integers(0, img.shape[0], n), rng.integers(0, img.shape[1], n)
        img[yy, xx] = np.where(rng.random(n) < 0.5, np.inf, -np.inf)
    small[40, 41], small[40, 42] = np.inf, -np.inf  # both signs inside one tap footprint
    lags = (truth["lag_crval1"] + np.arange(-4.0, 5.0, 2.0), truth["lag_crval2"] + np.arange(-4.0, 5.0, 2.0), None, None,
            [0.0, 0.3])
    with np.errstate(invalid="ignore"):
        want = H.oracle_carrington(small, hs, large, hl, lags, (72, 64), order=order)
        wanth = H.oracle_helio(small, hs, large, hl, lags, order=order)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (72, 64), order=order)
    H.assert_corr_close(got, want, 1e-10, f"carrington, Inf pixels, order {order}")
    goth = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
    H.assert_corr_close(goth, wanth, 1e-7, f"helioprojective, Inf pixels, order {order}")
    # and they do take samples out: the same sweep without them differs
    clean = H.gpu_carrington(gpu_handle, np.where(np.isfinite(small), small, 100.0), hs, large, hl, lags, (72, 64), order=order)
    assert np.nanmax(np.abs(clean - got)) > 1e-6


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 1), (2, 2), (3, 2), (2, 40), (40, 3)])
def test_images_of_a_few_pixels(gpu_handle, shape):
    """The smallest inputs: an axis of length 1 keeps no sample at all away from the zero lag (bounds rule c < 0 or
    c > n - 1, Util.py:98-102) and ONE at it -- the pixel at CRPIX, the only one wcslib's round trip returns exactly --
    whose centred sums are 0 / sqrt(0 * 0): NaN everywhere, in both frames and both helioprojective semantics; 2 x 2 and
    3 x 2 images give maps whose every sample has mirrored taps (and, with a handful of samples, lag-points the one-pass
    moments cannot carry); 2 x 40 and 40 x 3 images are all border: at the zero lag wcslib's rounding noise decides
    about EVERY pixel, and the lag-point is what is left after most of the sums have been taken out again."""
    from euispice_coreg_amd import synthetic
    ny, nx = shape
    small, hs, large, hl, _ = synthetic.make_scene(small_shape=shape, small_cdelt=(1008.0 / max(nx, 3), 1008.0 / max(ny, 3)),
                                                   large_n=96, seed=3, n_blobs=60, nan_frac=0.0)
    lags = ([-40.0, 0.0, 17.0, 90.0], [-9.0, 0.0, 60.0], None, None, [0.0, 0.3])
    for order in (1, 2, 3):
        with np.errstate(invalid="ignore", divide="ignore"):
            want = H.oracle_carrington(small, hs, large, hl, lags, (24, 20), order=order)
            wanth = H.oracle_helio(small, hs, large, hl, lags, order=order)
            wants = H.oracle_helio(small, hs, large, hl, lags, order=order, parallelism=False)
        if 1 in shape:
            assert np.isnan(want).all() and np.isnan(wanth).all() and np.isnan(wants).all()
        H.assert_corr_close(H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (24, 20), order=order), want, 1e-10,
                            f"carrington {shape} order {order}")
        H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order), wanth, 1e-7,
                            f"helioprojective sub-map {shape} order {order}")
        H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order, serial_semantics=True), wants,
                            1e-7, f"helioprojective full grid {shape} order {order}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 12), (9, 1), (2, 2), (3, 5)])
def test_carrington_grids_of_a_few_points(gpu_handle, shape):
    """Carrington grids down to one point (np.linspace(lo, hi, 1) = [lo], rectify.py:875-878): one grid point is one
    sample, NaN; a row, a column, 2 x 2 and 3 x 5 points give coefficients over a handful of samples (the re-evaluation
    about the lag-point's own means carries most of them)."""
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=96)
    lags = ([15.0, 17.0, 21.0], [-9.0, -5.0], None, None, [0.0, 0.3])
    for order in (1, 2, 3):
        with np.errstate(invalid="ignore", divide="ignore"):
            want = H.oracle_carrington(small, hs, large, hl, lags, shape, lonlims=(242.0, 249.0), latlims=(2.0, 8.0), order=order)
        if shape == (1, 1):
            assert np.isnan(want).all()
        else:
            assert np.isfinite(want).all()
        got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, lonlims=(242.0, 249.0), latlims=(2.0, 8.0),
                               order=order)
        H.assert_corr_close(got, want, 1e-10, f"carrington grid {shape} order {order}")


@pytest.mark.parametrize("large_n", [1, 2, 3])
def test_reference_images_of_a_few_pixels(gpu_handle, large_n):
    """A reference image of 1, 4 or 9 pixels: the once-only resampling (sub-map / Carrington transform) has mirrored taps
    everywhere or nothing in bounds at all; the full-grid helioprojective semantics correlate over at most 9 grid points."""
    small, hs, large, hl, _ = H.scene(small_n=48, large_n=large_n)
    lags = ([15.0, 17.0, 21.0], [-9.0, -5.0], None, None, [0.0, 0.3])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = H.oracle_helio(small, hs, large, hl, lags)
        wants = H.oracle_helio(small, hs, large, hl, lags, parallelism=False)
        wantc = H.oracle_carrington(small, hs, large, hl, lags, (16, 16))
    H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags), want, 1e-7, f"sub-map, large_n {large_n}")
    H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, serial_semantics=True), wants, 1e-7,
                        f"full grid, large_n {large_n}")
    H.assert_corr_close(H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (16, 16)), wantc, 1e-10,
                        f"carrington, large_n {large_n}")


def test_headers_that_cannot_give_pixel_coordinates_are_refused_before_any_launch(gpu_handle):
    """A NaN / infinite card, CDELT = 0, a singular PCi_j, a non-positive DSUN_OBS or solar radius, a non-finite lag or
    grid limit: COREG_EINVAL from every entry point that plans kernels from a header (the reference hands such a header to
    astropy, which raises, or returns NaN everywhere) -- and the handle keeps working afterwards.  A lag that makes
    CDELT + d_cdelt zero leaves its own lag-points NaN and nothing else."""
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene(small_n=48, large_n=64)
    h2 = _lib.CoregHandle(0)
    one = _lib.LagSet([0.0, 2.0], [0.0], None, None, None)
    grid = _lib.Grid((228.0, 262.0), (-12.0, 22.0), (40, 40))
    try:
        h2.set_small(small)
        h2.prepare_reference_helioprojective(large, hl, hs, 2)
        good = h2.sweep_helioprojective(hs, hs, one)
        bad_headers = [dict(hs, CDELT1=0.0), dict(hs, CDELT2=float("nan")), dict(hs, CRVAL1=float("inf")),
                       dict(hs, PC1_1=0.0, PC1_2=0.0), dict(hs, CRPIX2=float("nan")), dict(hs, PC2_1=float("nan")),
                       dict(hs, CRVAL1=1e300), dict(hs, CDELT2=1e-300)]  # (finite, but Inf - Inf a few products later)
        for bad in bad_headers:
            with pytest.raises(_lib.CoregError):
                h2.sweep_helioprojective(hs, bad, one)
            with pytest.raises(_lib.CoregError):
                h2.sweep_helioprojective(bad, hs, one)
            with pytest.raises(_lib.CoregError):
                h2.prepare_reference_helioprojective(large, bad, hs, 2)
            with pytest.raises(_lib.CoregError):
                h2.resample_helioprojective(hs, bad, 2)
        with pytest.raises(_lib.CoregError):
            h2.sweep_helioprojective(hs, hs, _lib.LagSet([0.0, float("nan")], [0.0], None, None, None))
        assert np.array_equal(h2.sweep_helioprojective(hs, hs, one), good)  # the handle is as it was
        h2.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        goodc = h2.sweep_carrington(hs, grid, 1.004, one)
        for bad in (dict(hs, DSUN_OBS=0.0), dict(hs, CRLN_OBS=float("nan")), dict(hs, CDELT1=0.0), dict(hs, CROTA=float("inf"))):
            with pytest.raises(_lib.CoregError):
                h2.sweep_carrington(bad, grid, 1.004, one)
            with pytest.raises(_lib.CoregError):
                h2.prepare_reference_carrington(large, bad, grid, 1.004, 2)
        with pytest.raises(_lib.CoregError):
            h2.sweep_carrington(hs, grid, 0.0, one)
        with pytest.raises(_lib.CoregError):
            h2.sweep_carrington(hs, _lib.Grid((228.0, float("nan")), (-12.0, 22.0), (40, 40)), 1.004, one)
        with pytest.raises(_lib.CoregError):  # 2.5e9 grid points: more than the 32-bit point lists hold
            h2.prepare_reference_carrington(large, hl, _lib.Grid((228.0, 262.0), (-12.0, 22.0), (50000, 50000)), 1.004, 2)
        h2.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        assert np.array_equal(h2.sweep_carrington(hs, grid, 1.004, one), goodc)
        # a CDELT1 lag of exactly -CDELT1 (intended semantics): that slice NaN, the others as without it
        lc = [-hs["CDELT1"], 0.0]
        got = h2.sweep_carrington(hs, grid, 1.004, _lib.LagSet([0.0, 2.0], [0.0], lc, None, None)).reshape(2, 1, 2)
        assert np.isnan(got[:, :, 0]).all() and np.array_equal(got[:, 0, 1], goodc.ravel())
    finally:
        h2.close()


# ---------------------------------------------------------------------------------------------------------------
def test_cfg1_against_committed_golden(gpu_handle):
    """BASELINE.json configs[0] (512^2 vs 1024^2, 11 x 11 CRVAL lags): GPU sweeps against the committed oracle
    output tests/golden/cfg1_corr.npz (made by tests/golden/make_golden_cfg1.py) -- serial semantics (full large
    grid, quirk Q1), parallel semantics (sub-map) and the Carrington frame."""
    import os
    from tests.conftest import GOLDEN
    from tests.golden import make_golden_cfg1 as G
    g = np.load(os.path.join(GOLDEN, "cfg1_corr.npz"))
    small, hs, large, hl, truth = G.scene()
    # same seeded inputs as when the fixture was made
    assert abs(np.nansum(small) - float(g["small_sum"])) <= 1e-6 * abs(float(g["small_sum"]))
    assert abs(np.nansum(large) - float(g["large_sum"])) <= 1e-6 * abs(float(g["large_sum"]))
    lags = G.lags(truth)
    assert np.array_equal(lags[0], g["lag_crval1"])
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, serial_semantics=True)
    H.assert_corr_close(got, g["serial"], 1e-7, "cfg1 serial semantics vs golden")
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags)
    H.assert_corr_close(got, g["parallel"], 1e-7, "cfg1 parallel semantics vs golden")
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (512, 512), (228.0, 262.0), (-12.0, 22.0))
    H.assert_corr_close(got, g["carrington"], 1e-10, "cfg1 carrington vs golden")
    am = np.unravel_index(np.nanargmax(got), got.shape)
    assert (lags[0][am[0]], lags[1][am[1]]) == (truth["lag_crval1"], truth["lag_crval2"])
    # BASELINE's own window, lag_crval1/2 in [-5, 5]: it contains the ZERO lag, whose border pixels on the sub-map path
    # are decided by wcslib's rounding noise (golden made by the oracle's WcslibTan, pinned by border_golden.npz)
    l0 = G.lags_baseline()
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, l0, serial_semantics=True)
    H.assert_corr_close(got, g["serial0"], 1e-7, "cfg1 [-5,5] serial semantics vs golden")
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, l0)
    H.assert_corr_close(got, g["parallel0"], 1e-7, "cfg1 [-5,5] parallel semantics vs golden")
    assert abs(got[5, 5, 0, 0, 0, 0] - g["parallel0"][5, 5, 0, 0, 0, 0]) <= 1e-7  # the zero lag itself
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, l0, (512, 512), (228.0, 262.0), (-12.0, 22.0))
    H.assert_corr_close(got, g["carrington0"], 1e-10, "cfg1 [-5,5] carrington vs golden")


def test_zero_lag_border_pixels_follow_wcslib(gpu_handle):
    """The zero lag of the sub-map path (target header == shifted header): the map is the identity up to wcslib's
    rounding noise and the sign of the noise decides, per border pixel, whether the bounds rule keeps it
    (alignment.py:1038-1069, utils/Util.py:98-102).  The library evaluates the round trip of the border pixels with
    wcslib's own arithmetic on the host and takes the dropped ones out of the six sums (k_border_fix): parity with
    the oracle at 1e-7 on 50-pixel images, where every border pixel weighs 1e-3 of the coefficient, for both
    orders, both methods, a rolled and an unrolled header and float32 / float64 pixels."""
    # (odd orders take floor(c) as their first tap: there the noise also decides, for EVERY pixel of such a lag-point,
    # which neighbour's NaN poisons the sample -- reproduced through per-pixel flags and k_parity_fix)
    for seed, crota, order, f32, nanf in ((3, 3.0, 2, True, 0.01), (4, 0.0, 1, False, 0.02), (5, -27.5, 2, False, 0.01),
                                          (6, 3.0, 3, True, 0.02), (7, 118.0, 1, True, 0.01)):
        small, hs, large, hl, _ = H.scene(small_n=50, large_n=96, seed=seed, float32_exact=f32, nan_frac=nanf)
        hs = dict(hs)
        rho = np.deg2rad(crota)
        hs["CROTA"] = crota
        hs["PC1_1"] = hs["PC2_2"] = float(np.cos(rho))
        hs["PC1_2"], hs["PC2_1"] = float(-np.sin(rho)), float(np.sin(rho))
        # CDELT-only lags at zero CRVAL lag leave one image axis invariant (rows for CDELT1, columns for CDELT2): their
        # border rows / columns are noise-decided too
        lags = (np.array([-4.0, 0.0, 4.0]), np.array([0.0, -3.0]), [0.0, 0.03], [0.0, -0.02], [0.0, 0.5])
        want = H.oracle_helio(small, hs, large, hl, lags, order=order)
        got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
        H.assert_corr_close(got, want, 1e-7, f"zero lag seed={seed}")
        # without the fix the zero lag keeps every border pixel: visibly different at this size
        gpu_handle.set_option("border_fix", 0)
        try:
            if order & 1:
                # odd orders have a second, general pass ("tap_fix": every sample within 1e-8 px of an integer -- the
                # bounds 0 and n - 1 are integers -- re-evaluated with wcslib's chain): it reproduces the oracle alone
                H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order), want, 1e-7,
                                    f"zero lag by the general pass, seed={seed}")
                # (round 5: of the 50 x 50 samples of that lag-point only those on the bounds rule or next to a NaN pixel
                # are listed -- the others cannot change the result; unfiltered, all of them are, with the same map)
                n_listed = gpu_handle.last_tap_fix()["samples"]
                assert 4 * 50 - 4 <= n_listed
                gpu_handle.set_option("tap_nan_filter", 0)
                try:
                    H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order), want, 1e-7,
                                        f"zero lag by the general pass, unfiltered, seed={seed}")
                    assert gpu_handle.last_tap_fix()["samples"] >= 50 * 50
                finally:
                    gpu_handle.set_option("tap_nan_filter", 2)
            else:
                # even orders: the bounds pass (samples within 1e-8 px of a bound of the image) does the same
                H.assert_corr_close(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order), want, 1e-7,
                                    f"zero lag by the bounds pass, seed={seed}")
                assert gpu_handle.last_tap_fix()["samples"] >= 4 * 50 - 4
            gpu_handle.set_option("tap_fix", 0)
            raw = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
        finally:
            gpu_handle.set_option("border_fix", 1)
            gpu_handle.set_option("tap_fix", 1)
        d = np.abs(raw - want)
        assert d[1, 0, 0, 0, 0, 0] > 1e-6
        # lag-points with a CRVAL or CROTA lag are not touched by the fix
        assert np.array_equal(raw[0], got[0]) and np.array_equal(raw[2], got[2]) and np.array_equal(raw[:, 1], got[:, 1])
        assert np.array_equal(raw[..., 1, :], got[..., 1, :])
    # the reference's own CDELT semantics: a CDELT1 lag only forces the PC rebuild -> identity up to the rebuilt PC's
    # last bit, still decided by wcslib's noise
    lags = (np.array([0.0, 4.0]), np.array([0.0]), [0.0, 0.03], None, None)
    want = H.oracle_helio(small, hs, large, hl, lags, cdelt_semantics="reference")
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, cdelt_semantics=1)
    H.assert_corr_close(got, want, 1e-7, "zero lag, reference CDELT semantics")


@pytest.mark.parametrize("order", [0, 3, 4, 5])
def test_other_spline_orders_vs_oracle(gpu_handle, order):
    """reprojection_order is a user argument (alignment.py:54) and scipy's map_coordinates takes 0..5: the orders the
    tuned kernels do not cover run on the run-time-order variant (global-memory gather), all three frames."""
    small, hs, large, hl, _ = H.scene(small_n=72, large_n=112)
    lags = _lags(4, 3, crota=[0.0, 0.3])
    want = H.oracle_carrington(small, hs, large, hl, lags, (40, 36), order=order)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (40, 36), order=order)
    H.assert_corr_close(got, want, 1e-9, f"carrington order={order}")
    for serial in (False, True):
        want = H.oracle_helio(small, hs, large, hl, lags, order=order, parallelism=not serial)
        got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order, serial_semantics=serial)
        H.assert_corr_close(got, want, 1e-7, f"helio order={order} serial={serial}")
    from euispice_coreg_amd import _lib, synthetic
    cs, chs, cl, chl, _ = synthetic.make_car_scene(small_shape=(60, 70), large_shape=(90, 100))
    clags = (np.array([0.0, 0.018]), np.array([-0.011, 0.004]), None, None, None)
    gpu_handle.set_small(cs)
    gpu_handle.set_reference_on_grid(np.asarray(cl, dtype=np.float32))
    ls = _lib.LagSet(*clags)
    got = gpu_handle.sweep_helioprojective(chl, chs, ls, order=order).reshape(ls.shape + (1,))
    want = H.oracle_helio(cs.astype(np.float64), chs, cl.astype(np.float64), chl, clags, order=order, parallelism=False,
                          unit_lag="deg")
    H.assert_corr_close(got, want, 1e-7, f"CAR order={order}")


def test_spline_order_out_of_range_is_an_error(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene(small_n=32, large_n=48)
    with pytest.raises(_lib.CoregError):
        H.gpu_helio(gpu_handle, small, hs, large, hl, _lags(2, 2), order=6)


@pytest.mark.parametrize("serial", [False, True])
def test_sweep_helioprojective_unsorted_lag_lists(gpu_handle, serial):
    """The reference takes lag lists in any order (alignment.py:667-674 meshes them as given).  With the serial
    semantics (target = full large grid) the cull box of the precompute decides which grid points exist: it must cover
    the extreme lags BY VALUE, wherever they sit in the list."""
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=128)
    lags = (np.array([0.0, -24.0, 38.0, -8.0, 16.0, 29.0]), np.array([3.0, 31.0, -27.0, -9.0, 12.0]), None, None,
            [0.3, 0.0])
    want = H.oracle_helio(small, hs, large, hl, lags, parallelism=not serial)
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, serial_semantics=serial)
    H.assert_corr_close(got, want, 1e-7, f"helio unsorted lags serial={serial}")
    # and the sorted sweep holds the same numbers at the permuted positions
    o1, o2 = np.argsort(lags[0]), np.argsort(lags[1])
    srt = H.gpu_helio(gpu_handle, small, hs, large, hl, (lags[0][o1], lags[1][o2], None, None, [0.0, 0.3]),
                      serial_semantics=serial)
    assert np.allclose(srt, got[o1][:, o2][:, :, :, :, ::-1], rtol=0, atol=1e-12, equal_nan=True)


def test_sweep_carrington_unsorted_lag_lists(gpu_handle):
    small, hs, large, hl, _ = H.scene()
    lags = (np.array([17.0, -11.0, 25.0, 3.0]), np.array([-9.0, 19.0, -23.0, 5.0, -1.0]), None, None, None)
    want = H.oracle_carrington(small, hs, large, hl, lags, (72, 64))
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (72, 64))
    H.assert_corr_close(got, want, 1e-10, "carrington unsorted lags")


def test_tile_skip_is_exact_on_a_coarse_limb_crossing_grid(gpu_handle):
    """k_precompute drops whole tiles whose (Lipschitz-bounded) image misses the cull box.  The bound is provable, so
    the kept-point count and the map must be IDENTICAL with the skip switched off -- checked on a coarse grid that
    crosses the limb and is much wider than the small field of view (most tiles are skipped), with long thin tiles."""
    small, hs, large, hl, _ = H.scene(small_n=96, large_n=160)
    lags = (17.0 + 3.0 * (np.arange(6) - 3), -9.0 + 3.0 * (np.arange(5) - 2), None, None, [0.0, 0.4])
    lon, lat, shape = (150.0, 350.0), (-89.0, 89.0), (700, 300)
    res = {}
    for tw in (0, 256, 4):
        gpu_handle.set_option("tile_w", tw)
        try:
            for skip in (1, 0):
                gpu_handle.set_option("tile_skip", skip)
                got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, lonlims=lon, latlims=lat)
                res[(tw, skip)] = (got, gpu_handle.last_stats()["n_active_points"])
        finally:
            gpu_handle.set_option("tile_skip", 1)
            gpu_handle.set_option("tile_w", 0)
        assert res[(tw, 1)][1] == res[(tw, 0)][1] > 0
        assert np.array_equal(res[(tw, 1)][0], res[(tw, 0)][0], equal_nan=True)
    want = H.oracle_carrington(small, hs, large, hl, lags, shape, lonlims=lon, latlims=lat)
    H.assert_corr_close(res[(0, 1)][0], want, 1e-10, "coarse limb-crossing grid")


def test_point_sharded_sweeps_add_up_to_the_unsharded_map(gpu_handle):
    """Multi-GPU mode for few lag-points per GPU (SURVEY 8e fallback): every rank sweeps ALL the lags over its share of
    the grid's points and the six sums per lag are added (one all-reduce).  Emulated here on one GPU: the W ranks'
    sums, added on the host and finalised, equal the unsharded map -- Carrington with several (cdelt, crota)
    launches, helioprojective through the zero lag (whose border correction only rank 0 carries), method 'residus'."""
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = H.scene()
    lags = _lags(5, 4, cdelt1=[0.0, 0.02], crota=[0.0, 0.3])
    ls = _lib.LagSet(*lags)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (72, 64))
    full = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (72, 64)).ravel()
    for W in (2, 3, 8):
        total = None
        try:
            for r in range(W):
                gpu_handle.set_point_shard(r, W)
                nanmap = gpu_handle.sweep_carrington(hs, grid, 1.004, ls)
                assert np.isnan(nanmap).all()  # a sharded sweep returns no coefficients by itself
                s = gpu_handle.copy_sums()
                total = s if total is None else total + s
            got = gpu_handle.finalize_sums(total, ls.size)
        finally:
            gpu_handle.set_point_shard(0, 1)
        assert np.abs(got - full).max() <= 1e-12, W
    # a slice of the lag range, sharded
    try:
        total = None
        for r in range(2):
            gpu_handle.set_point_shard(r, 2)
            gpu_handle.sweep_carrington(hs, grid, 1.004, ls, lag_begin=7, lag_end=61)
            s = gpu_handle.copy_sums()
            total = s if total is None else total + s
        got = gpu_handle.finalize_sums(total, 61 - 7)
    finally:
        gpu_handle.set_point_shard(0, 1)
    assert np.abs(got - full[7:61]).max() <= 1e-12
    # helioprojective, lag axes through exactly zero (sub-map semantics), both methods
    small, hs, large, hl, _ = H.scene(small_n=50, large_n=96, seed=3)
    lags = (np.array([-4.0, 0.0, 4.0]), np.array([0.0, -3.0]), None, None, [0.0, 0.5])
    ls = _lib.LagSet(*lags)
    for method in (0, 1):
        gpu_handle.set_small(small if method == 0 else np.nan_to_num(small, nan=100.0))
        gpu_handle.prepare_reference_helioprojective(large, hl, hs, 2)
        full = gpu_handle.sweep_helioprojective(hs, hs, ls, method=method)
        try:
            total = None
            for r in range(4):
                gpu_handle.set_point_shard(r, 4)
                gpu_handle.sweep_helioprojective(hs, hs, ls, method=method)
                s = gpu_handle.copy_sums()
                total = s if total is None else total + s
            got = gpu_handle.finalize_sums(total, ls.size)
        finally:
            gpu_handle.set_point_shard(0, 1)
        assert np.allclose(got, full, rtol=0, atol=1e-12, equal_nan=True), method
    # calling the finaliser without a pending sharded sweep is an error
    with pytest.raises(_lib.CoregError):
        gpu_handle.sweep_helioprojective(hs, hs, ls)
        gpu_handle.finalize_sums(np.zeros(6), 1)


@pytest.mark.parametrize("W", [2, 4])
def test_point_sharded_sweeps_re_evaluate_ill_conditioned_lag_points_like_one_gpu(gpu_handle, W):
    """VERDICT r04 missing 3: grid shares across GPUs used to skip the re-evaluation of ill-conditioned lag-points, so
    an N-GPU map could differ from the 1-GPU map (and from c_correlate.py:39-72) on exactly those.  Now the flags come
    from the REDUCED sums and every rank re-evaluates the flagged lag-points over the whole grid (coreg_finalize_sums;
    the compacted points of earlier launches are computed again).  (i) the six-active-point case of seed 80246, two
    (cdelt) launches; (ii) every lag-point of a three-launch sweep forced through the re-evaluation."""
    from euispice_coreg_amd import _lib
    from tests.test_gpu_fuzz import _random_case

    def sharded(hs_, grid_, ls_, solar_r=1.004):
        total = None
        try:
            for r in range(W):
                gpu_handle.set_point_shard(r, W)
                gpu_handle.sweep_carrington(hs_, grid_, solar_r, ls_)
                s_ = gpu_handle.copy_sums()
                total = s_ if total is None else total + s_
            return gpu_handle.finalize_sums(total, ls_.size)
        finally:
            gpu_handle.set_point_shard(0, 1)

    small, hs, large, hl, lags, _ = _random_case(80246)
    lags = list(lags)
    lags[3] = [0.0, -0.02]
    g = dict(shape=(23, 25), lonlims=(200.0, 234.0), latlims=(-72.0, 22.0))
    want = H.oracle_carrington(small, hs, large, hl, lags, g["shape"], g["lonlims"], g["latlims"], order=2,
                               solar_r=(1.004,))
    one = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, order=2, **g)
    n_one = gpu_handle.last_visit_counts()["refined_lag_points"]
    assert n_one > 0
    ls = _lib.LagSet(*lags)
    grid = _lib.Grid(g["lonlims"], g["latlims"], g["shape"])
    got = sharded(hs, grid, ls).reshape(one.shape)
    assert gpu_handle.last_visit_counts()["refined_lag_points"] > 0
    H.assert_corr_close(got, want, 1e-13, f"ill-conditioned lag-points, {W} grid shares")
    assert np.array_equal(np.isnan(got), np.isnan(one)) and np.nanmax(np.abs(got - one)) <= 1e-13
    # (ii) three launches (crota), every lag-point flagged: the earlier launches' points are re-computed
    small, hs, large, hl, _ = H.scene()
    lags = _lags(5, 4, crota=[0.0, 0.3, -0.2])
    ls = _lib.LagSet(*lags)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (72, 64))
    gpu_handle.set_option("refine_cond_log10", -1)
    try:
        one = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (72, 64)).ravel()
        assert gpu_handle.last_visit_counts()["refined_lag_points"] == ls.size
        got = sharded(hs, grid, ls)
        assert gpu_handle.last_visit_counts()["refined_lag_points"] == ls.size
    finally:
        gpu_handle.set_option("refine_cond_log10", 5)
    assert np.abs(got - one).max() <= 1e-13
    H.assert_corr_close(got.reshape(ls.shape + (1,)), H.oracle_carrington(small, hs, large, hl, lags, (72, 64)), 1e-10,
                        f"every lag-point re-evaluated, {W} grid shares")


@pytest.mark.parametrize("order", [1, 2])
def test_all_finite_windows_take_the_unmasked_path_and_agree(gpu_handle, order):
    """Interior visits whose LDS window holds no NaN skip the per-sample mask and take the count and the reference
    moments from per-chunk sums (kernels.hpp: point_lag CLEAN): same map as the masked arithmetic up to summation
    rounding, on both geometries, and the oracle's map on an image with a NaN block (windows of both kinds)."""
    small, hs, large, hl, _ = H.scene(small_n=192, large_n=200, nan_frac=0.0)
    lags = _lags(9, 8, step=1.5)
    shape = (160, 144)
    inner = dict(lonlims=(240.0, 250.0), latlims=(0.0, 10.0))  # a grid well inside the field of view: interior tiles
    maps, counts = {}, {}
    for clean in (1, 0):
        gpu_handle.set_option("clean_path", clean)
        gpu_handle.set_option("tile_w", 16)
        try:
            c = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, shape, order=order, **inner)
            counts[clean] = [gpu_handle.last_visit_counts()]
            hp = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
            counts[clean].append(gpu_handle.last_visit_counts())
            maps[clean] = (c, hp)
        finally:
            gpu_handle.set_option("clean_path", 1)
            gpu_handle.set_option("tile_w", 0)
    for k in (0, 1):
        assert counts[1][k]["interior"] > 0 and counts[1][k]["all_finite"] == counts[1][k]["interior"], counts
        assert counts[0][k]["interior"] == counts[1][k]["interior"] and counts[0][k]["all_finite"] == 0, counts
        assert np.array_equal(np.isnan(maps[1][k]), np.isnan(maps[0][k]))
        assert np.nanmax(np.abs(maps[1][k] - maps[0][k])) <= 1e-13
    H.assert_corr_close(maps[1][0], H.oracle_carrington(small, hs, large, hl, lags, shape, order=order, **inner), 1e-10,
                        "carrington, all-finite image")
    H.assert_corr_close(maps[1][1], H.oracle_helio(small, hs, large, hl, lags, order=order), 1e-7,
                        "helioprojective, all-finite image")
    # a NaN block: windows that touch it keep the mask, the others do not
    holed = small.copy()
    holed[60:100, 80:140] = np.nan
    gpu_handle.set_option("tile_w", 16)
    try:
        got = H.gpu_carrington(gpu_handle, holed, hs, large, hl, lags, shape, order=order, **inner)
        cc = gpu_handle.last_visit_counts()
        got_h = H.gpu_helio(gpu_handle, holed, hs, large, hl, lags, order=order)
        ch = gpu_handle.last_visit_counts()
    finally:
        gpu_handle.set_option("tile_w", 0)
    assert 0 < cc["all_finite"] < cc["interior"], cc
    assert ch["all_finite"] < ch["interior"], ch
    H.assert_corr_close(got, H.oracle_carrington(holed, hs, large, hl, lags, shape, order=order, **inner), 1e-10,
                        "carrington, NaN block")
    H.assert_corr_close(got_h, H.oracle_helio(holed, hs, large, hl, lags, order=order), 1e-7,
                        "helioprojective, NaN block")


def test_ill_conditioned_lag_points_are_re_evaluated_with_centred_sums(gpu_handle):
    """Six active grid points, lag-points with a handful of samples whose coefficient is +-1 by construction: the
    one-pass formula about the global pivots loses seven digits there (1.6e-9 on this case, tests/deep_fuzz.py seed
    80246); k_finalize notices and re-evaluates those lag-points the way c_correlate.py:39-72 does."""
    from tests.test_gpu_fuzz import _random_case
    small, hs, large, hl, lags, _ = _random_case(80246)
    lags = list(lags)
    lags[3] = [0.0, -0.02]
    grid = dict(shape=(23, 25), lonlims=(200.0, 234.0), latlims=(-72.0, 22.0), order=2)
    want = H.oracle_carrington(small, hs, large, hl, lags, grid["shape"], grid["lonlims"], grid["latlims"], order=2,
                               solar_r=(1.004,))
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, **grid)
    counts = gpu_handle.last_visit_counts()
    assert gpu_handle.last_stats()["n_active_points"] == 6
    assert counts["refined_lag_points"] > 0, counts
    H.assert_corr_close(got, want, 1e-13, "ill-conditioned lag-points, refined")
    gpu_handle.set_option("refine", 0)
    try:
        raw = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, **grid)
        assert gpu_handle.last_visit_counts()["refined_lag_points"] == 0
    finally:
        gpu_handle.set_option("refine", 1)
    assert np.array_equal(np.isnan(raw), np.isnan(want))
    assert 1e-10 < np.nanmax(np.abs(raw - want)) < 1e-7  # what the one-pass formula gives here
    # a well-conditioned sweep is not touched
    small, hs, large, hl, _ = H.scene()
    H.gpu_carrington(gpu_handle, small, hs, large, hl, _lags(7, 6), (72, 64))
    assert gpu_handle.last_visit_counts()["refined_lag_points"] == 0


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("finite_border", [False, True])
def test_ill_conditioned_lag_points_are_re_evaluated_next_to_a_zero_lag_too(gpu_handle, finite_border, order):
    """A helioprojective sweep THROUGH the zero lag (whose noise-decided samples are taken out of / put into the sums by
    an extra slab) over data the one-pass moments cannot carry: a nearly flat reference on the image's own grid
    (1000 +- 1e-3) with a block at -1e7 where the image to align is masked -- it moves the pivot, never overlaps.  Every
    lag-point is flagged, the zero lag included, and every one is re-evaluated about its own means and gives the two-pass
    coefficient of c_correlate.py:39-72: for a launch with a slab the fix kernels run a second time, about the flagged
    slots' own pivots, into a slab of the re-evaluation (until round 5 such a launch was never re-evaluated).
    `finite_border`: the zero lag really has border samples to take out (masked border: nothing to take out); odd
    orders add the pixels whose tap set the sign of wcslib's noise decides (scattered NaN pixels)."""
    from euispice_coreg_amd import _lib
    from oracle import coreg_oracle as O
    rng = np.random.default_rng(8)
    small, hs, _, hl, _ = H.scene(small_n=64, large_n=96, nan_frac=0.01)
    small = small.copy()
    small[:8, :8] = np.nan          # the pivot-moving block of the reference sits under masked pixels ...
    if not finite_border:
        small[[0, -1], :] = np.nan
        small[:, [0, -1]] = np.nan
    ref = 1000.0 + 1.0e-3 * rng.standard_normal(small.shape)
    ref[:6, :6] = -1.0e7            # ... and away from their tap footprints
    lags = ([-2.0, 0.0, 2.0], [-2.0, 0.0, 2.0], None, None, None)
    st = H.oracle_state(small, hs, ref, hl, lags, order=order)
    want = O.find_best_header_parameters(st, "helioprojective", prepared_reference=ref)[..., 0].reshape(3, 3)
    assert np.isfinite(want).all() and np.abs(want).max() < 0.2  # noise against structure
    ls = _lib.LagSet(*lags)
    gpu_handle.set_small(small)
    gpu_handle.set_reference_on_grid(ref)
    got = gpu_handle.sweep_helioprojective(hs, hs, ls, order=order).reshape(3, 3)
    counts = gpu_handle.last_visit_counts()
    assert counts["refined_lag_points"] == 9 and counts["flagged_not_refined"] == 0, counts
    assert np.abs(got - want).max() <= 1e-7, np.abs(got - want)
    gpu_handle.set_option("refine", 0)
    try:
        raw = gpu_handle.sweep_helioprojective(hs, hs, ls, order=order).reshape(3, 3)
    finally:
        gpu_handle.set_option("refine", 1)
    assert not np.nanmax(np.abs(raw - want)) <= 1e-4  # what the one-pass formula gives on these data
    # grid shares across GPUs (two and three ranks, emulated on this handle): the flags come from the REDUCED sums,
    # every rank re-evaluates over the whole grid and runs the launch's fix kernels a second time itself
    for world in (2, 3):
        total = None
        try:
            for r in range(world):
                gpu_handle.set_point_shard(r, world)
                gpu_handle.sweep_helioprojective(hs, hs, ls, order=order)
                part = gpu_handle.copy_sums()
                total = part if total is None else total + part
            shared = gpu_handle.finalize_sums(total, ls.size).reshape(3, 3)
        finally:
            gpu_handle.set_point_shard(0, 1)
        assert gpu_handle.last_visit_counts()["refined_lag_points"] == 9
        assert np.abs(shared - want).max() <= 1e-7 and np.abs(shared - got).max() <= 1e-10, (world, np.abs(shared - got))
    if finite_border:
        # and the zero lag's noise-decided samples do matter at this level: without them it is off
        gpu_handle.set_option("border_fix", 0)
        gpu_handle.set_option("tap_fix", 0)
        try:
            nofix = gpu_handle.sweep_helioprojective(hs, hs, ls, order=order).reshape(3, 3)
        finally:
            gpu_handle.set_option("border_fix", 1)
            gpu_handle.set_option("tap_fix", 1)
        assert np.abs(nofix - want)[1, 1] > 1e-7 and np.abs(np.delete((nofix - want).ravel(), 4)).max() <= 1e-7


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("f32_exact", [True, False])
def test_re_evaluating_every_lag_point_gives_the_oracle_map(gpu_handle, order, f32_exact):
    """The re-evaluation of flagged lag-points (k_refine: sums about the lag-point's own means) forced onto EVERY lag-point (threshold 0.1): all three
    frames, compile-time and run-time spline orders, float32 and float64 pixels, CROTA / CDELT lags -- the maps the
    oracle gives, and the maps of the one-pass sums to summation rounding."""
    small, hs, large, hl, _ = H.scene(small_n=72, large_n=112, float32_exact=f32_exact)
    lags = _lags(4, 3, crota=[0.0, 0.3], cdelt1=[0.0, 0.03])
    from euispice_coreg_amd import _lib, synthetic
    cs, chs, cl, chl, _ = synthetic.make_car_scene(small_shape=(60, 70), large_shape=(90, 100))
    clags = (np.array([0.0, 0.018]), np.array([-0.011, 0.004]), None, None, None)
    cls = _lib.LagSet(*clags)

    def run_all():
        out = [H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, (40, 36), order=order)]
        n_ref = [gpu_handle.last_visit_counts()["refined_lag_points"]]
        # (lags that do not pass through zero: no noise-decided border pixels, whose launches are not re-evaluated)
        out.append(H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order))
        n_ref.append(gpu_handle.last_visit_counts()["refined_lag_points"])
        gpu_handle.set_small(cs)
        gpu_handle.set_reference_on_grid(np.asarray(cl, dtype=np.float32))
        out.append(gpu_handle.sweep_helioprojective(chl, chs, cls, order=order).reshape(cls.shape + (1,)))
        n_ref.append(gpu_handle.last_visit_counts()["refined_lag_points"])
        return out, n_ref

    one_pass, n0 = run_all()
    gpu_handle.set_option("refine_cond_log10", -1)
    try:
        two_pass, n1 = run_all()
    finally:
        gpu_handle.set_option("refine_cond_log10", 5)
    assert n0 == [0, 0, 0]
    for k, (a, b) in enumerate(zip(one_pass, two_pass)):
        assert n1[k] == int(np.isfinite(b).sum()) or n1[k] >= int(np.isfinite(b).sum()), (k, n1)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.nanmax(np.abs(a - b)) <= 1e-12, (k, np.nanmax(np.abs(a - b)))
    H.assert_corr_close(two_pass[0], H.oracle_carrington(small, hs, large, hl, lags, (40, 36), order=order), 1e-9,
                        f"carrington order={order}, every lag-point re-evaluated")
    H.assert_corr_close(two_pass[1], H.oracle_helio(small, hs, large, hl, lags, order=order), 1e-7,
                        f"helio order={order}, every lag-point re-evaluated")
    H.assert_corr_close(two_pass[2], H.oracle_helio(cs.astype(np.float64), chs, cl.astype(np.float64), chl, clags, order=order,
                                                    parallelism=False, unit_lag="deg"), 1e-7,
                        f"CAR order={order}, every lag-point re-evaluated")
