"""GPU tests of method "mutual_information" on the Carrington header-shift sweep (include/coreg_hip.h:
coreg_sweep_set_bins; csrc/kernels_sweep_mi.hpp), against the numpy oracle of tests/hdrshift_mi_oracle.py.

The rule of every parity case.  The library and the oracle run the same arithmetic in another order, so a value agrees to
its rounding (1e-16 relative) and a coordinate to 1e-12 px: wherever no kept value lies within 1e-8 (relative) of an edge
and no sample coordinate within 1e-9 px of a bound of the image -- asserted FIRST, with the oracle's `margins`; a case
that did not meet it would be re-seeded, not loosened -- the two histograms are identical.  Then the counts must be equal
exactly and |MI - oracle| <= 1e-11 (ATOL of tests/test_gpu_pxlshift_mi.py: identical histograms, only `log` differs)
with the same NaN pattern, and the argmax equal wherever the oracle's best two entries differ by more than 2 ATOL."""
import warnings

import numpy as np
import pytest

from tests import hdrshift_mi_oracle as MO
from tests import helpers as H
from tests.test_gpu_masked_scores import _lags, carr_state

pytestmark = pytest.mark.gpu

ATOL = 1e-11
EDGE_MARGIN, BOUND_MARGIN = 1e-8, 1e-9
MI = "mutual_information"


def _edges(small, ref, n_small, n_large=None):
    from euispice_coreg_amd.pxlshift.alignment_pixels import quantile_edges
    return quantile_edges(small, n_small), quantile_edges(ref, n_small if n_large is None else n_large)


def _reference(scene, shape, order=2, **grid):
    from oracle import coreg_oracle as O
    small, hs, large, hl = scene[:4]
    st = carr_state(small, hs, large, hl, _lags(1, 1), shape, **grid)
    st.order = order
    return O.prepare_reference(st, "carrington", 1.004, True)


def _oracle(scene, lags, shape, es, el, order=2, what="", **grid):
    """The oracle's sweep, its precondition asserted: {"mi", "count"} raveled in C order."""
    small, hs, large, hl = scene[:4]

    def state():
        st = carr_state(small, hs, large, hl, lags, shape, **grid)
        st.order = order
        return st
    edge, bound = MO.margins(state(), es, el)
    print(f"\n[hdrshift mi] {what}: smallest relative distance to an edge {edge:.2e}, to a bound {bound:.2e} px")
    assert edge > EDGE_MARGIN and bound > BOUND_MARGIN, (what, edge, bound)
    want = MO.sweep(state(), "carrington", es, el)
    return {k: v.ravel() for k, v in want.items()}


def _sweep(h, scene, lags, shape, es, el, order=2, prepare=True, method=None, lon=H.CARR_LON, lat=H.CARR_LAT, **kw):
    """(cube, counts) of one sweep through the C ABI (edges None: the handle's)."""
    from euispice_coreg_amd import _lib
    small, hs, large, hl = scene[:4]
    grid = _lib.Grid(lon, lat, shape)
    if prepare:
        h.set_small(small)
        h.prepare_reference_carrington(large, hl, grid, 1.004, order)
    if es is not None:
        h.sweep_set_bins(es, el)
    got = h.sweep_carrington(hs, grid, 1.004, _lib.LagSet(*lags), order=order,
                             method=_lib.METHOD_MUTUAL_INFORMATION if method is None else method, **kw)
    return got, h.last_counts()


def _check(got, n_got, want, what):
    got, n_got = np.asarray(got, dtype=np.float64).ravel(), np.asarray(n_got, dtype=np.float64).ravel()
    mi, n = np.asarray(want["mi"]).ravel(), np.asarray(want["count"]).ravel()
    assert got.shape == mi.shape == n_got.shape, (what, got.shape, mi.shape)
    assert np.array_equal(n_got, n), f"{what}: counts differ\n{n_got}\n{n}"
    assert np.array_equal(np.isnan(got), np.isnan(mi)), f"{what}: NaN pattern differs\n{got}\n{mi}"
    fin = np.isfinite(mi)
    if not fin.any():
        return
    err = np.abs(got[fin] - mi[fin]).max()
    print(f"\n[hdrshift mi] {what}: max |MI - oracle| = {err:.3e} (bound {ATOL:.0e}), counts {n.min():.0f} .. {n.max():.0f}")
    assert err <= ATOL, f"{what}: {err:.3e}"
    top = np.sort(mi[fin])[::-1]
    if top.size > 1 and top[0] - top[1] > 2 * ATOL:
        assert np.nanargmax(got) == np.nanargmax(mi), f"{what}: argmax differs"


@pytest.fixture(scope="module")
def usual():
    """The usual scene with the oracle's reference on the usual grid (two tiles) and on (96, 80)."""
    scene = H.scene()[:4]
    return scene, _reference(scene, (48, 40)), _reference(scene, (96, 80))


# ---- 1. the usual grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [4, 8, 16, "3x31"])
def test_usual_grid(gpu_handle, usual, bins):
    """4, 8 and 16 quantile bins, and a lopsided pair with 3 and 31 edges (32 bins on one side); the counts are also the
    Pearson sweep's on the same handle, entry for entry."""
    from euispice_coreg_amd import _lib
    scene, ref, _ = usual
    small = scene[0]
    es, el = _edges(small, ref, 4, 32) if bins == "3x31" else _edges(small, ref, bins)
    assert (len(es), len(el)) == ((3, 31) if bins == "3x31" else (bins - 1, bins - 1))
    lags = _lags(5, 5)
    want = _oracle(scene, lags, (48, 40), es, el, what=f"usual grid, bins {bins}")
    assert want["count"].min() == 780 and want["count"].max() == 788 and np.isfinite(want["mi"]).all()
    got, n = _sweep(gpu_handle, scene, lags, (48, 40), es, el)
    _check(got, n, want, f"usual grid, bins {bins}")
    assert gpu_handle.last_stats()["n_sweep_launches"] == 1
    corr, n_corr = _sweep(gpu_handle, scene, lags, (48, 40), None, None, prepare=False, method=_lib.METHOD_CORRELATION)
    assert np.isfinite(corr).all() and np.array_equal(n_corr, n)


# ---- 2. 32 x 32 bins: 64 KiB of LDS histograms -------------------------------------------------------------------------
def test_32_x_32_bins(gpu_handle, usual):
    scene, _, ref = usual
    es, el = _edges(scene[0], ref, 32)
    assert len(es) == len(el) == 31
    lags = _lags(5, 5)
    want = _oracle(scene, lags, (96, 80), es, el, what="32 x 32 bins, (96, 80)")
    assert want["count"].min() == 3193 and want["count"].max() == 3215
    got, n = _sweep(gpu_handle, scene, lags, (96, 80), es, el)
    _check(got, n, want, "32 x 32 bins, (96, 80)")


# ---- 3. spline orders, float32 and float64 pixels ----------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_orders_and_pixel_types(gpu_handle, usual, order):
    """Every k_sweep_mi instantiation: orders 1, 2 and 3 (the run-time order), the image to align resident as float32 and
    as float64.  The library keeps every float32-exact image as float32, so the float64 copy has ONE pixel moved by one
    ulp of float64 (1e-16 relative: eight orders of magnitude inside the precondition's margin, no sample changes its
    bin): the two cubes must be identical, counts included."""
    scene, _, _ = usual
    small, hs, large, hl = scene
    ref = _reference(scene, (48, 40), order=order)
    es, el = _edges(small, ref, 8)
    lags = _lags(5, 5)
    want = _oracle(scene, lags, (48, 40), es, el, order=order, what=f"order {order}")
    got, n = _sweep(gpu_handle, scene, lags, (48, 40), es, el, order=order)
    assert gpu_handle.last_stats()["small_is_f32"] == 1
    _check(got, n, want, f"order {order}, float32 pixels")
    moved = small.copy()
    at = np.unravel_index(np.flatnonzero(np.isfinite(small))[small.size // 3], small.shape)
    moved[at] = np.nextafter(small[at], np.inf)
    assert moved[at] != small[at] and np.float64(np.float32(moved[at])) != moved[at]
    got64, n64 = _sweep(gpu_handle, (moved, hs, large, hl), lags, (48, 40), es, el, order=order)
    assert gpu_handle.last_stats()["small_is_f32"] == 0
    assert np.array_equal(got64, got, equal_nan=True) and np.array_equal(n64, n)


# ---- 4. four launches, ragged slot groups: slices, combination shares, chunk counts ----------------------------------
def test_slices_shares_and_chunks_are_bit_identical(gpu_handle, usual):
    """7 x 5 CRVAL lags (35 slots: three groups of 16, the last ragged) x 2 CDELT2 x 2 CROTA lags = four launches.  The
    whole cube against the oracle; a lag slice, a share of the combinations and 1, 2 and 5 chunks of the tile list give
    the same bits, counts included."""
    scene, ref, _ = usual
    es, el = _edges(scene[0], ref, 8)
    lags = _lags(7, 5, cdelt2=[0.0, 0.02], crota=[0.0, 0.3])
    want = _oracle(scene, lags, (48, 40), es, el, what="four launches")
    whole, n = _sweep(gpu_handle, scene, lags, (48, 40), es, el)
    assert gpu_handle.last_stats()["n_sweep_launches"] == 4 and whole.size == 140
    _check(whole, n, want, "four launches")
    part, n_part = _sweep(gpu_handle, scene, lags, (48, 40), None, None, prepare=False, lag_begin=3, lag_end=19)
    assert np.array_equal(part, whole[3:19]) and np.array_equal(n_part, n[3:19])
    gpu_handle.set_option("combo_begin", 1)
    gpu_handle.set_option("combo_end", 3)
    share, n_share = _sweep(gpu_handle, scene, lags, (48, 40), None, None, prepare=False, lag_begin=0, lag_end=70)
    assert np.array_equal(share, whole.reshape(7, 5, 4)[:, :, 1:3].ravel())
    assert np.array_equal(n_share, n.reshape(7, 5, 4)[:, :, 1:3].ravel())
    try:
        for chunks in (1, 2, 5):
            gpu_handle.set_option("mi_chunks", chunks)
            again, n_again = _sweep(gpu_handle, scene, lags, (48, 40), None, None, prepare=False)
            assert np.array_equal(again, whole) and np.array_equal(n_again, n), chunks
    finally:
        gpu_handle.set_option("mi_chunks", 0)


# ---- 5. masking ---------------------------------------------------------------------------------------------------------
def test_masking_and_a_lag_off_the_image(gpu_handle, usual):
    """A NaN block and an infinite pixel in the image to align, NaN in the reference image; one lag slides the grid off the
    image: MI NaN, count 0, and `min_overlap` removes it."""
    from euispice_coreg_amd.hdrshift.alignment import apply_min_overlap
    small, hs, large, hl = (np.array(a) if isinstance(a, np.ndarray) else a for a in usual[0])
    small[30:41, 22:37] = np.nan
    small[60, 50] = np.inf
    large[70:78, 80:90] = np.nan
    scene = (small, hs, large, hl)
    ref = _reference(scene, (48, 40))
    assert np.isnan(ref).sum() > np.isnan(usual[1]).sum()
    es, el = _edges(small, ref, 8)
    lags = (np.array([13.0, 17.0, 21.0, 30017.0]), np.array([-11.0, -7.0]), None, None, None)
    want = _oracle(scene, lags, (48, 40), es, el, what="masking")
    off = want["count"] == 0
    assert off.sum() == 2 and np.array_equal(off, np.isnan(want["mi"])) and want["count"][~off].min() > 600
    assert want["count"][~off].max() < 780  # (the blocks take pairs away)
    got, n = _sweep(gpu_handle, scene, lags, (48, 40), es, el)
    _check(got, n, want, "masking")
    kept = apply_min_overlap(got, n, 0.5)
    assert np.array_equal(np.isnan(kept), off) and np.array_equal(kept[~off], got[~off])
    # every lag off the image: the map is refused by min_overlap, not returned as a row of NaN
    gone, n_gone = _sweep(gpu_handle, scene, (np.array([30017.0]), np.array([-9.0]), None, None, None), (48, 40), None, None,
                          prepare=False)
    assert np.isnan(gone).all() and (n_gone == 0).all()
    with pytest.raises(ValueError):
        apply_min_overlap(gone, n_gone, 0.5)


# ---- 6. the ABI ---------------------------------------------------------------------------------------------------------
def _code(fn, *args, **kw):
    from euispice_coreg_amd import _lib
    with pytest.raises(_lib.CoregError) as e:
        fn(*args, **kw)
    return e.value.code


def test_refusals_by_error_code(usual):
    from euispice_coreg_amd import _lib
    scene, ref, _ = usual
    small, hs, large, hl = scene
    es, el = _edges(small, ref, 8)
    lags, ls = _lags(3, 3), _lib.LagSet(*_lags(3, 3))
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    ok = np.arange(1.0, 32.0)
    with _lib.CoregHandle(0) as h:
        before, n_before = _sweep(h, scene, lags, (48, 40), None, None, method=_lib.METHOD_CORRELATION)
        run = lambda: h.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_MUTUAL_INFORMATION)  # noqa: E731
        assert _code(run) == _lib.COREG_ESTATE  # no bins set
        h.pixels_set_bins(es, el)               # (the pixel-lag sweep's lists are another state)
        assert _code(run) == _lib.COREG_ESTATE
        for bad in ([], np.arange(32.0), [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf]):
            assert _code(h.sweep_set_bins, bad, ok) == _lib.COREG_EINVAL
            assert _code(h.sweep_set_bins, ok, bad) == _lib.COREG_EINVAL
        assert _code(run) == _lib.COREG_ESTATE  # still none
        h.sweep_set_bins(es, el)
        cube = run()
        n_cube = h.last_counts()
        _check(cube, n_cube, _oracle(scene, lags, (48, 40), es, el, what="3 x 3 lags"), "3 x 3 lags")
        for bad in ([], np.arange(32.0), [2.0, 1.0]):
            assert _code(h.sweep_set_bins, bad, ok) == _lib.COREG_EINVAL
            assert _code(h.sweep_set_bins, ok, bad) == _lib.COREG_EINVAL
        assert np.array_equal(run(), cube) and np.array_equal(h.last_counts(), n_cube)  # the earlier lists still hold
        # the other sweeps have no such score
        h.prepare_reference_helioprojective(large, hl, hs, 2)
        assert _code(h.sweep_helioprojective, hs, hs, ls, method=_lib.METHOD_MUTUAL_INFORMATION) == _lib.COREG_ENOTIMPL
        assert _code(h.sweep_context, hs, hs, np.zeros(hs["NAXIS1"], dtype=np.int32), ls,
                     method=_lib.METHOD_MUTUAL_INFORMATION) == _lib.COREG_ENOTIMPL
        assert _code(h.sweep_helioprojective, hs, hs, ls, method=7) == _lib.COREG_ENOTIMPL
        assert _code(h.set_option, "mi_chunks", 65) == _lib.COREG_EINVAL and _code(h.set_option, "mi_chunks", -1) == _lib.COREG_EINVAL
        # a grid share
        h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        h.set_point_shard(1, 2)
        try:
            assert _code(run) == _lib.COREG_ENOTIMPL
        finally:
            h.set_point_shard(0, 1)
        assert np.array_equal(run(), cube)
        # the Pearson sweep after a mutual-information sweep: the bits it had before
        after, n_after = _sweep(h, scene, lags, (48, 40), None, None, prepare=False, method=_lib.METHOD_CORRELATION)
        assert np.array_equal(after, before) and np.array_equal(n_after, n_before)


# ---- 7. through the classes -----------------------------------------------------------------------------------------------
LON, LAT, SHAPE = (236.0, 256.0), (-4.0, 16.0), (96, 96)


@pytest.fixture(scope="module")
def folded():
    """`synthetic.make_scene` (10 000 blobs: the median lies inside the structure) with the image to align passed through
    |log(x / median)| plus noise -- bright and faint structure alike give large values, no linear relation to the
    reference is left -- on a grid inside the field of view, 7 x 7 lags of about one pixel about the injected (17, -9)."""
    from oracle import coreg_oracle as O
    small, hs, large, hl, truth = H.scene(small_n=96, large_n=1024, seed=6, n_blobs=10000, pointing_error=(17.0, -9.0, 0.0))
    rng = np.random.default_rng(7)
    small = np.abs(np.log(small / np.nanmedian(small))) + 0.05 * rng.standard_normal(small.shape)
    small = small.astype(np.float32).astype(np.float64)
    lags = (17.0 + 10.0 * (np.arange(7) - 3), -9.0 + 10.0 * (np.arange(7) - 3), None, None, None)
    scene = (small, hs, large, hl)
    ref = _reference(scene, SHAPE, lon=LON, lat=LAT)
    es, el = _edges(small, ref, 8)
    want = MO.sweep(carr_state(small, hs, large, hl, lags, SHAPE, lon=LON, lat=LAT), "carrington", es, el)
    pearson = O.find_best_header_parameters(carr_state(small, hs, large, hl, lags, SHAPE, lon=LON, lat=LAT), "carrington")
    return scene, lags, (es, el), want, pearson


def test_the_classes_find_the_lag_the_pearson_coefficient_misses(folded, tmp_path):
    from euispice_coreg_amd.hdrshift import Alignment, AlignmentResults
    scene, lags, (es, el), want, pearson = folded
    small, hs, large, hl = scene
    # the test's own precondition, on the CPU oracle: MI peaks at the injected lag, well above the rest; Pearson does not
    mi = want["mi"][..., 0, 0, 0, 0]
    best = np.unravel_index(np.nanargmax(mi), mi.shape)
    top = np.sort(mi.ravel())[::-1]
    assert best == (3, 3) and (lags[0][3], lags[1][3]) == (17.0, -9.0) and top[0] - top[1] > 0.3
    p = pearson[..., 0, 0, 0, 0]
    assert np.unravel_index(np.nanargmax(p), p.shape) != (3, 3) and p[3, 3] < 0.0
    assert want["count"].min() > 0.5 * want["count"].max()
    kw = dict(lonlims=LON, latlims=LAT, shape=SHAPE)
    A = Alignment((large, hl), (small, hs), lag_crval1=lags[0], lag_crval2=lags[1], lag_cdelt1=None, lag_cdelt2=None,
                  lag_crota=None, min_overlap=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = A.align_using_carrington(method=MI, bins=8, **kw)
    assert isinstance(res, AlignmentResults) and res.best == "max" and res.corr.shape == (7, 7, 1, 1, 1, 1)
    assert tuple(int(v) for v in res.max_index)[:2] == (3, 3)
    assert np.isfinite(res.corr).all() and np.isfinite(A.last_counts).all() and np.isfinite(res.shift_arcsec).all()
    assert np.array_equal(A.last_counts, want["count"]) and np.array_equal(res.n_samples, want["count"])
    # the default edges: the quantiles of the image and of the library's own reference on the grid (the oracle's to rounding)
    assert len(A.last_bins) == 2 and np.array_equal(A.last_bins[0], es) and np.allclose(A.last_bins[1], el, rtol=1e-12, atol=0)
    # explicit edges through the class: the oracle's bits to ATOL
    B = Alignment((large, hl), (small, hs), lag_crval1=lags[0], lag_crval2=lags[1], lag_cdelt1=None, lag_cdelt2=None,
                  lag_crota=None)
    corr = B.align_using_carrington(method=MI, bins=(es, el), return_type="corr", **kw)
    assert np.array_equal(B.last_bins[0], es) and np.array_equal(B.last_bins[1], el)
    edge, bound = MO.margins(carr_state(small, hs, large, hl, lags, SHAPE, lon=LON, lat=LAT), es, el)
    assert edge > EDGE_MARGIN and bound > BOUND_MARGIN, (edge, bound)
    _check(corr, B.last_counts, want, "through the class, explicit edges")
    # the Pearson sweep of the same object misses, as the oracle said it would
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rp = B.align_using_carrington(method="correlation", **kw)
    assert tuple(int(v) for v in rp.max_index)[:2] != (3, 3)
    with pytest.raises(ValueError):
        B.align_using_carrington(method="correlation", bins=8, **kw)


def test_spice_and_jitter_take_the_keywords(tmp_path):
    """`AlignmentSpice.align_using_carrington` and `jitter_correction_imagers` hand `method` / `bins` on."""
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    from euispice_coreg_amd.jitter_correction import jitter_correction_imagers
    from euispice_coreg_amd.utils import fits_io
    cube, h4, large, hl, truth = synthetic.make_spice_l2()
    lag1, lag2 = np.arange(-31.0, -14.0, 4.0), np.arange(28.0, 45.0, 4.0)
    S = AlignmentSpice((large, hl), (cube, h4), lag_crval1=lag1, lag_crval2=lag2, parallelism=True, level=2)
    kw = dict(lonlims=(241.0, 247.0), latlims=(3.5, 9.0), shape=(60, 110))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = S.align_using_carrington(method=MI, bins=6, **kw)
    assert res.best == "max" and res.corr.shape == (5, 5, 1, 1, 1, 1) and np.isfinite(res.corr).all()
    assert len(S.last_bins[0]) == len(S.last_bins[1]) == 5 and np.isfinite(S.last_counts).all()
    es, el = S.last_bins
    want = MO.sweep(carr_state(S.data_small, S.hdr_small, large, hl, (lag1, lag2, None, None, None), kw["shape"],
                               lon=kw["lonlims"], lat=kw["latlims"]), "carrington", es, el)
    assert np.array_equal(S.last_counts, want["count"])
    assert np.unravel_index(np.nanargmax(res.corr), res.corr.shape) == np.unravel_index(np.nanargmax(want["mi"]), want["mi"].shape)
    with pytest.raises(ValueError):
        S.align_using_carrington(method="correlation", bins=6, **kw)
    # the jitter series of tests/test_gpu_masked_scores.py, two frames
    frames, _ = synthetic.make_series(n_frames=2, n=256, seed=7, jitter_sigma=4.0)
    paths = []
    for k, (img, hdr) in enumerate(frames):
        p = str(tmp_path / f"solo_L2_eui-hrieuv174-image_{k:03d}.fits")
        fits_io.write_images(p, [(None, {}), (img, hdr)])
        paths.append(p)
    lag = np.arange(-8.0, 8.5, 4.0)
    done = jitter_correction_imagers(paths, str(tmp_path / "out"), lonlims=(236.0, 256.0), latlims=(-4.0, 16.0), shape=(100, 100),
                                     lag_crval1=lag, lag_crval2=lag, sublist_length=2, overlap=1, method=MI, bins=8,
                                     min_overlap=0.5)
    assert [(a, r) for a, r, _ in done] == [(1, 0)]
    res = done[0][2]
    assert res.best == "max" and res.corr.shape == (5, 5, 1, 1, 1, 1) and np.isfinite(res.corr).all()
