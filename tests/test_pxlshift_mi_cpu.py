"""
CPU tests of the mutual-information score of the pixel-lag alignment (pxlshift): the numpy
restatement tests/pxlshift_mi_oracle.py against figures worked out by hand, the default-edge rule and the refusals of
`bins` and of the method through `host_plan`, and a scene on which the new score finds the injected lag and the Pearson
coefficient does not.  No GPU.
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.hdrshift import Alignment
from euispice_coreg_amd.hdrshift.alignment import library_method
from euispice_coreg_amd.pxlshift import AlignmentPixels, LocalShiftField, PixelAlignmentResults
from euispice_coreg_amd.pxlshift.alignment_pixels import check_edges, quantile_edges, zero_lag_window

from . import helpers as H
from . import pxlshift_cases as Cs
from . import pxlshift_mi_oracle as M
from . import pxlshift_oracle as O
from . import pxlshift_scores_oracle as S
from .pxlshift_tiles_cases import HDR


# ------------------------------------------------------------------------------------------------ the oracle, by hand
def test_a_two_by_two_histogram():
    # n = 8, every margin 4: two cells of 3 at ratio 3 * 8 / 16, two of 1 at ratio 8 / 16
    want = 2 * (3 / 8) * np.log(1.5) + 2 * (1 / 8) * np.log(0.5)
    assert abs(M.mi_of_histogram([[3, 1], [1, 3]]) - want) <= 1e-16
    assert abs(want - 0.13081203594113694) <= 1e-15
    assert abs(M.mi_of_histogram([[4, 0], [0, 4]]) - np.log(2.0)) <= 1e-16
    # the same through the pixels: edges (0.5) and (10), pairs placed cell by cell
    a = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    b = np.array([9.0, 9.0, 9.0, 11.0, 9.0, 11.0, 11.0, 11.0])
    assert np.array_equal(M.histogram(a, b, [0.5], [10.0]), [[3, 1], [1, 3]])
    mi, n = M.entry(a, b, [0.5], [10.0])
    assert n == 8 and abs(mi - want) <= 1e-16


def test_independent_margins_give_zero():
    hist = np.outer([2, 3, 5], [1, 4, 2, 7])  # n_ij n = r_i c_j in every cell
    assert abs(M.mi_of_histogram(hist)) <= 1e-16
    assert M.mi_of_histogram([[0, 0, 0], [5, 2, 9]]) == 0.0  # one row
    assert M.mi_of_histogram([[0, 5], [0, 2], [0, 9]]) == 0.0  # one column


@pytest.mark.parametrize("B", [2, 8, 32])
def test_identical_images_with_equally_filled_bins_give_log_b(B):
    v = np.random.default_rng(3).permutation(np.arange(B * 12, dtype=np.float64)).reshape(12, B)
    edges = np.arange(1, B) * 12.0  # 12 values per bin
    hist = M.histogram(v, v, edges, edges)
    assert np.array_equal(hist, 12 * np.eye(B, dtype=np.int64))
    mi, n = M.entry(v, v, edges, edges)
    assert n == 12 * B and abs(mi - np.log(B)) <= 4e-16 * np.log(B) * B


def test_edges_infinities_and_nan():
    edges = [1.0, 2.0, 4.0]
    v = np.array([0.999, 1.0, np.nextafter(2.0, 0.0), 2.0, 4.0, np.inf, -np.inf, 1e300])
    # a value on an edge belongs to the bin above it; +-inf fall into the end bins
    assert np.array_equal(np.searchsorted(edges, v, side="right"), [0, 1, 1, 2, 3, 3, 0, 3])
    hist = M.histogram(v, v, edges, edges)
    assert np.array_equal(np.diag(hist), [2, 2, 1, 3]) and hist.sum() == 8
    a = np.array([np.nan, 1.5, np.inf, 3.0])
    b = np.array([1.5, np.nan, 0.0, -np.inf])
    hist = M.histogram(a, b, edges, edges)
    assert hist.sum() == 2 and hist[3, 0] == 1 and hist[2, 0] == 1  # a NaN on either side drops the pair, an inf does not
    mi, n = M.entry([np.nan, 1.0], [1.0, np.nan], edges, edges)
    assert n == 0 and np.isnan(mi)


# ------------------------------------------------------------------------------------------------ the default edges
def test_quantile_edges():
    v = np.arange(1.0, 101.0)
    assert np.array_equal(quantile_edges(v, 4), np.quantile(v, [0.25, 0.5, 0.75]))
    assert len(quantile_edges(v, 32)) == 31
    ties = np.array([1.0] * 90 + [2.0] * 5 + [np.nan] * 3 + [np.inf, -np.inf, 7.0])
    e = quantile_edges(ties, 16)  # the finite pixels: 90 ones, five twos, a seven; most quantiles are 1.0
    assert e[0] == 1.0 and len(e) < 6 and np.all(np.diff(e) > 0) and np.all(np.isfinite(e))
    assert np.array_equal(quantile_edges(np.full((5, 4), 3.5), 16), [3.5])  # a constant image: one edge
    with pytest.raises(ValueError):
        quantile_edges(np.array([np.nan, np.inf, -np.inf]), 8)


@pytest.mark.parametrize("name", ["a", "b"])
def test_default_edges_come_from_the_zero_lag_window(name, tmp_path):
    A, kw = Cs.make(name, tmp_path)
    p = A.host_plan(**kw, method="mutual_information")
    r1, r2 = p["ratio_res_1"], p["ratio_res_2"]
    assert (r1, r2) == ((0.9, 0.8) if name == "a" else (1.3, 0.7))  # a: up-sampled, b: down-sampled along the columns
    (h, w), (l0, l1) = A.data_small.shape, p["slc_small_ref"]
    rows, cols = zero_lag_window(A.data_large.shape, (h, w), (l0, l1), r1, r2)
    assert (rows.start, rows.stop - 1) == (int(np.floor(l0 * r2)), int(np.ceil((l0 + h - 1) * r2)))
    assert (cols.start, cols.stop - 1) == (int(np.floor(l1 * r1)), int(np.ceil((l1 + w - 1) * r1)))
    assert rows.stop <= A.data_large.shape[0] and cols.stop <= A.data_large.shape[1]
    es, el = p["bins"]
    fin = A.data_small[np.isfinite(A.data_small)]
    assert np.array_equal(es, np.unique(np.quantile(fin, np.arange(1, 16) / 16)))
    win = A.data_large[rows, cols]
    assert np.array_equal(el, np.unique(np.quantile(win[np.isfinite(win)], np.arange(1, 16) / 16)))
    assert p["method_code"] == _lib.METHOD_MUTUAL_INFORMATION == 3
    # the edges do not depend on the lag lists
    q = A.host_plan(kw["lag_dx"][:2], kw["lag_dy"][-1:], kw["lag_drot"][:1], unit_rot=kw["unit_rot"],
                    method="mutual_information")
    assert np.array_equal(q["bins"][0], es) and np.array_equal(q["bins"][1], el)
    # a window clipped to the image
    rows, cols = zero_lag_window((10, 12), (8, 30), (5, -2), 1.5, 1.0)
    assert (rows.start, rows.stop, cols.start, cols.stop) == (5, 10, 0, 12)


def test_no_finite_pixel(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    A.data_small[:] = np.nan
    with pytest.raises(ValueError):
        A.host_plan(**kw, method="mutual_information")
    assert len(A.host_plan(**kw, method="mutual_information", bins=([1.0], [2.0]))["bins"][0]) == 1


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    for method in ("correlation", "residus_masked"):
        for bins in (16, ([1.0], [2.0])):
            with pytest.raises(ValueError):
                A.host_plan(**kw, method=method, bins=bins)
    ok = np.arange(1.0, 32.0)
    bad_lists = ([], np.arange(32.0), [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf], [[1.0, 2.0]], ["a"], 3.0)
    bad = [1, 33, 0, -4, True, 16.0, "16", (ok,), (ok, ok, ok)]
    bad += [(b, ok) for b in bad_lists] + [(ok, b) for b in bad_lists]
    for bins in bad:
        with pytest.raises(ValueError):
            A.host_plan(**kw, method="mutual_information", bins=bins)
    for b in bad_lists:
        with pytest.raises(ValueError):
            check_edges(b, "edges")
    for bins in (2, 32, np.int64(8), (ok, [0.5]), ([0.5], ok)):
        p = A.host_plan(**kw, method="mutual_information", bins=bins)
        assert all(e.dtype == np.float64 and 1 <= len(e) <= 31 for e in p["bins"])
    with pytest.raises(ValueError):
        A.find_best_parameters(**kw, bins=8)  # (refused before any GPU work)
    with pytest.raises(ValueError):
        A.find_local_shifts(**kw, tile_shape=(10, 9), bins=8)
    # the header-shift paths have no such method: what an unknown method raises there
    with pytest.raises(NotImplementedError):
        library_method("mutual_information")
    with pytest.raises(NotImplementedError):
        library_method("no-such-method")
    small, hs, large, hl, _ = H.scene(small_n=32, large_n=32)
    for method in ("mutual_information", "no-such-method"):  # through a class: refused before any GPU work
        with pytest.raises(NotImplementedError):
            Alignment((large, hl), (small, hs), [0.0], [0.0], None, None, None).align_using_helioprojective(method=method)
    # the result classes know the method: best = maximum
    x, y = np.meshgrid(np.arange(9.0), np.arange(7.0), indexing="ij")
    cube = (1.4 * np.exp(-((x - 4.3) ** 2 / 4.0 + (y - 2.6) ** 2 / 3.0)))[:, :, None]
    R = PixelAlignmentResults(cube, np.arange(9), np.arange(7), [0.0], method="mutual_information")
    assert R.best == "max" and R.max_index == (4, 3, 0) and abs(R.shift_pixels[0] - 4.3) < 1e-5
    F = LocalShiftField(cube[None, None], np.full((1, 1, 9, 7, 1), 9.0), np.arange(9), np.arange(7), [0.0], (3, 3), (3, 3),
                        method="mutual_information", sub_lag=False)
    assert F.best == "max" and tuple(F.best_index[0, 0]) == (4, 3, 0)


# ------------------------------------------------------------------------------------------------ where it is needed
def scene_object(bins=8):
    large, small, kw = M.scene(seed=1, shape=(24, 20), lag=(-2, 3))
    return AlignmentPixels((large, dict(HDR)), 0, (small, dict(HDR)), 0), kw, bins


def test_the_score_finds_a_lag_the_correlation_misses():
    """|log(x / median)| of a log-normal image, noise, a NaN block: seed 1, 24 x 20 pixels, 8 bins, lag (-2, 3)."""
    A, kw, bins = scene_object()
    o = M.scores(A.data_large, A.data_small, A.host_plan(**kw, method="mutual_information", bins=bins))
    mi = o["mi"]
    true = (int(np.nonzero(kw["lag_dx"] == -2)[0][0]), int(np.nonzero(kw["lag_dy"] == 3)[0][0]), 0)
    top = np.sort(mi.ravel())[::-1]
    corr = S.scores(A.data_large, A.data_small, A.host_plan(**kw))["corr"]
    best_corr = np.unravel_index(np.nanargmax(corr), corr.shape)
    print("MI best", top[0], "second", top[1], "Pearson best", corr[best_corr], "at", best_corr, "at the lag", corr[true])
    assert np.unravel_index(np.nanargmax(mi), mi.shape) == true
    assert top[0] - top[1] >= 0.3
    assert best_corr != true
    assert o["count"][true] == 24 * 20 - 12


def test_oracle_takes_prepared_planes_and_box(tmp_path):
    A, kw = Cs.make("a", tmp_path)
    p = A.host_plan(**kw, method="mutual_information", bins=8)
    own = M.scores(A.data_large, A.data_small, p)
    sub = O.sub_resolution(A.data_large, p["ratio_res_1"], p["ratio_res_2"])
    (h, w), (l0, l1) = A.data_small.shape, p["slc_small_ref"]
    dx, dy = p["lag_dx"], p["lag_dy"]
    box = sub[l0 + dy.min():l0 + dy.max() + h, l1 + dx.min():l1 + dx.max() + w]
    planes = [O.rotate(A.data_small, d, p["unit_rot"]) for d in p["lag_drot"]]
    given = M.scores(None, A.data_small, p, planes=planes, box=box)
    assert np.array_equal(own["mi"], given["mi"], equal_nan=True) and np.array_equal(own["count"], given["count"])
    tiled = M.scores(A.data_large, A.data_small, p, tile_shape=(10, 9))
    assert tiled["mi"].shape == (3, 3) + own["mi"].shape
    assert np.array_equal(tiled["count"].sum(axis=(0, 1)), own["count"])
    whole = M.scores(A.data_large, A.data_small, p, tile_shape=A.data_small.shape)
    assert np.array_equal(whole["mi"][0, 0], own["mi"], equal_nan=True)
