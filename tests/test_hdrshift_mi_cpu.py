"""
CPU tests of the mutual-information score of the Carrington header-shift sweep (include/coreg_hip.h: coreg_sweep_set_bins,
DESIGN section 8): the `bins` argument and its refusals through `Alignment.align_using_carrington`, the default-edge rule,
the numpy oracle tests/hdrshift_mi_oracle.py (its mask is the Pearson sums'; the score is invariant under increasing maps
of both images with mapped edges), and the refusals the other frames keep.  No GPU.
"""
import inspect

import numpy as np
import pytest

from euispice_coreg_amd import synthetic
from euispice_coreg_amd.hdrshift import Alignment
from euispice_coreg_amd.hdrshift import alignment as AL
from euispice_coreg_amd.pxlshift.alignment_pixels import quantile_edges
from oracle import coreg_oracle as O

from . import helpers as H
from . import hdrshift_mi_oracle as MO
from . import masked_scores_oracle as M
from .pxlshift_mi_oracle import mi_of_histogram

GRID = dict(lonlims=H.CARR_LON, latlims=H.CARR_LAT, shape=(48, 40))
LAGS = (17.0 + 2.0 * (np.arange(3) - 1), -9.0 + 2.0 * (np.arange(3) - 1), None, None, None)


@pytest.fixture(scope="module")
def scene():
    return H.scene()


def _state(scene, lags=LAGS):
    small, hs, large, hl, _ = scene
    return H.oracle_state(small, hs, large, hl, lags, shape=[48, 40], lonlims=list(H.CARR_LON), latlims=list(H.CARR_LAT),
                          solar_r=(1.004,))


def _alignment(scene, **kw):
    small, hs, large, hl, _ = scene
    return Alignment((large, hl), (small, hs), [0.0, 2.0], [0.0], None, None, None, **kw)


# ------------------------------------------------------------------------------------------------ `bins` and its refusals
def test_bins_belong_to_mutual_information(scene):
    """[new] Refused with ValueError before anything is loaded, hence before any GPU work (this machine has no GPU: a
    sweep that started would raise something else)."""
    for method in ("correlation", "residus", "residus_masked"):
        for bins in (8, ([1.0], [2.0])):
            with pytest.raises(ValueError):
                _alignment(scene).align_using_carrington(method=method, bins=bins, **GRID)
            with pytest.raises(ValueError):
                AL.parse_bins(method, bins)
        assert AL.parse_bins(method, None) is None


def test_bad_bins_are_refused_before_any_gpu_work(scene):
    """[new] The bad `bins` of tests/test_pxlshift_mi_cpu.py::test_refusals, through `align_using_carrington`."""
    ok = np.arange(1.0, 32.0)
    bad_lists = ([], np.arange(32.0), [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf], [[1.0, 2.0]], ["a"], 3.0)
    bad = [1, 33, 0, -4, True, 16.0, "16", (ok,), (ok, ok, ok)]
    bad += [(b, ok) for b in bad_lists] + [(ok, b) for b in bad_lists]
    for bins in bad:
        with pytest.raises(ValueError):
            _alignment(scene).align_using_carrington(method="mutual_information", bins=bins, **GRID)
    assert AL.parse_bins("mutual_information", None) == AL.DEFAULT_BINS == 16 and AL.MAX_BINS == 32
    for bins in (2, 32, np.int64(8)):
        assert AL.parse_bins("mutual_information", bins) == int(bins)
    for bins in ((ok, [0.5]), ([0.5], ok)):
        es, el = AL.parse_bins("mutual_information", bins)
        assert es.dtype == el.dtype == np.float64 and 1 <= len(es) <= 31 and 1 <= len(el) <= 31


# ------------------------------------------------------------------------------------------------ the default edges
def test_default_edges_are_plain_numpy_on_images_and_thresholds(scene):
    """[new] Quantiles of the image to align after its thresholds and of the reference on the grid: no lag list, slice or
    rank is among the arguments, and two `Alignment` objects with different lag lists hand it the same ones."""
    small, hs, large, hl, _ = scene
    assert list(inspect.signature(AL.default_edges).parameters) == ["small_pixels", "value_min", "value_max",
                                                                    "reference_on_grid", "n_bins"]
    ref = O.prepare_reference(_state(scene), "carrington", 1.004, True)
    es, el = AL.default_edges(small, None, None, ref, 8)
    assert np.array_equal(es, quantile_edges(small, 8)) and np.array_equal(el, quantile_edges(ref, 8))
    assert len(es) == len(el) == 7 and es.dtype == el.dtype == np.float64
    again = AL.default_edges(small.copy(), None, None, O.prepare_reference(_state(scene, (LAGS[0][:1], [0.0, 5.0, 9.0], None,
                                                                                         None, None)), "carrington", 1.004, True), 8)
    assert np.array_equal(again[0], es) and np.array_equal(again[1], el)
    # thresholds: the pixels they remove do not enter the quantiles; the caller's image is left alone
    fin = small[np.isfinite(small)]
    lo, hi = float(np.quantile(fin, 0.2)), float(np.quantile(fin, 0.7))
    before = small.copy()
    et, _ = AL.default_edges(small, lo, hi, ref, 8)
    assert np.array_equal(small, before, equal_nan=True)
    cut = small.astype(np.float64)
    O.set_threshold_minmax_to_nan(cut, lo, hi)
    assert np.array_equal(et, quantile_edges(cut, 8)) and et[0] >= lo and et[-1] <= hi and not np.array_equal(et, es)
    with pytest.raises(ValueError):
        AL.default_edges(np.full((4, 4), np.nan), None, None, ref, 8)


# ------------------------------------------------------------------------------------------------ the oracle
def test_the_oracle_counts_the_pairs_of_the_pearson_sums(scene):
    small, hs, _, _, _ = scene
    st = _state(scene)
    es, el = quantile_edges(small, 8), quantile_edges(O.prepare_reference(st, "carrington", 1.004, True), 8)
    got = MO.sweep(_state(scene), "carrington", es, el)
    assert got["mi"].shape == got["count"].shape == (3, 3, 1, 1, 1, 1) and np.isfinite(got["mi"]).all()
    O.set_initial_header_values(st, True)
    table, _ = O.lag_table(st)
    A = O.prepare_reference(st, "carrington", 1.004, True)
    for i, lg in enumerate(table):
        hdr = dict(st.hdr_small)
        O.shift_header(st, hdr, *lg)
        B = O.carrington_transform_fa(st.data_small, hdr, 1.004, st.shape, st.lonlims, st.latlims, st.order)
        assert got["count"].ravel()[i] == M.pearson_count(A, B) > 700
        # an infinite value is dropped, as the Pearson mask drops it (the pixel-lag oracle keeps it)
        B2 = B.copy()
        B2.ravel()[np.flatnonzero(np.isfinite(B.ravel()) & np.isfinite(A.ravel()))[0]] = np.inf
        assert MO.histogram(A, B2, es, el).sum() == M.pearson_count(A, B) - 1
    assert np.array_equal(got["count"], M.sweep(_state(scene), "carrington")["count"])
    assert np.isnan(mi_of_histogram(MO.histogram(A, np.full_like(A, np.nan), es, el)))


def test_increasing_maps_with_mapped_edges_leave_the_score_alone(scene):
    small, hs, _, _, _ = scene
    st = _state(scene)
    O.set_initial_header_values(st, True)
    table, _ = O.lag_table(st)
    A = O.prepare_reference(st, "carrington", 1.004, True)
    es, el = quantile_edges(small, 8), quantile_edges(A, 16)

    def f(v):  # (exact in floating point: strictly increasing on the doubles)
        return 8.0 * np.asarray(v, dtype=np.float64)

    def g(v):  # (a product of monotone roundings: increasing, strictly so on values a few ulps apart)
        v = np.asarray(v, dtype=np.float64)
        return v * v * v

    for lg in table[::4]:
        hdr = dict(st.hdr_small)
        O.shift_header(st, hdr, *lg)
        B = O.carrington_transform_fa(st.data_small, hdr, 1.004, st.shape, st.lonlims, st.latlims, st.order)
        hist = MO.histogram(A, B, es, el)
        assert hist.sum() > 700 and np.array_equal(hist, MO.histogram(f(A), g(B), g(es), f(el)))
        assert mi_of_histogram(hist) == mi_of_histogram(MO.histogram(f(A), g(B), g(es), f(el))) > 0.0


# ------------------------------------------------------------------------------------------------ the other frames
def test_the_other_frames_keep_refusing_the_method(scene):
    small, hs, large, hl, _ = scene
    with pytest.raises(NotImplementedError):
        AL.library_method("mutual_information")
    assert "mutual_information" not in AL._METHODS and AL.MUTUAL_INFORMATION == "mutual_information"
    for method in ("mutual_information", "no-such-method"):  # refused before any GPU work
        with pytest.raises(NotImplementedError):
            Alignment((large, hl), (small, hs), [0.0], [0.0], None, None, None).align_using_helioprojective(method=method)
    with pytest.raises(NotImplementedError, match="align_using_carrington"):
        Alignment((large, hl), (small, hs), [0.0], [0.0], None, None, None).align_using_helioprojective(
            method="mutual_information")
    cs, chs, cl, chl, _ = synthetic.make_car_scene()
    with pytest.raises(NotImplementedError, match="align_using_carrington"):
        Alignment((cl, chl), (cs, chs), [0.0], [0.0], None, None, None).align_using_initial_carrington(
            method="mutual_information")
    with pytest.raises(NotImplementedError):
        Alignment((large, hl), (small, hs), [0.0], [0.0], None, None, None).align_using_carrington(
            method="no-such-method", **GRID)
