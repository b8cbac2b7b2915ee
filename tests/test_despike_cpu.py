"""
The median/MAD despiking without a GPU: properties of the oracle (tests/despike_oracle.py, the rule in numpy), the forms a
`despike_small=` / `despike_large=` keyword may take (utils/despiking.py) with every ValueError, the classes refusing a bad
keyword before they load a file, and the seeded scene the feature is for.
"""
import inspect

import numpy as np
import pytest

from euispice_coreg_amd.utils.despiking import DEFAULTS, despike_params, despike_tag
from tests import despike_oracle as DO


def _flat(shape=(9, 11), value=100.0, dtype=np.float64):
    return np.full(shape, value, dtype=dtype)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_image_flags_nothing(dtype):
    v = _flat(dtype=dtype)
    out, counts = DO.despike(v, n_iter=3)
    assert counts == [0, 0, 0] and np.array_equal(out, v) and out.dtype == dtype
    out, counts = DO.despike(v, n_iter=1, sign="both", nsigma=1e-6)  # mad = 0, floor = 0: scale = 0 decides nothing
    assert counts == [0] and np.array_equal(out, v)


def test_the_floor_alone_decides_on_a_flat_neighbourhood():
    v = _flat()
    v[4, 5] = 110.0
    assert DO.despike(v, n_iter=1)[1] == [0]                       # scale = 0: kept however large the step
    assert DO.despike(v, n_iter=1, floor=2.5)[1] == [0]            # d = 10 is not > 5 * 2.5
    out, counts = DO.despike(v, n_iter=1, floor=1.9)               # ... but > 5 * 1.9
    assert counts == [1] and np.isnan(out[4, 5]) and np.isfinite(out).sum() == v.size - 1
    out, counts = DO.despike(v, n_iter=1, floor=2.0)               # d > nsigma * scale is strict
    assert counts == [0]


def test_sign():
    v = _flat()
    v[2, 3], v[6, 7] = 160.0, 40.0
    out, counts = DO.despike(v, n_iter=1, floor=1.0)
    assert counts == [1] and np.isnan(out[2, 3]) and out[6, 7] == 40.0
    out, counts = DO.despike(v, n_iter=1, floor=1.0, sign="both")
    assert counts == [2] and np.isnan(out[2, 3]) and np.isnan(out[6, 7])


def test_replace_median_rounds_to_the_images_dtype():
    rng = np.random.default_rng(3)
    v64 = 100.0 + rng.uniform(0.0, 1.0, (9, 11))  # medians that no float32 holds
    v64[4, 5] = 500.0
    out, counts = DO.despike(v64, n_iter=1, replace="median")
    nb = np.delete(v64[2:7, 3:8].ravel(), 12)
    s = np.sort(nb)
    med = (s[11] + s[12]) * 0.5
    assert counts == [1] and out[4, 5] == med and out.dtype == np.float64
    changed = out != v64
    assert changed.sum() == 1 and changed[4, 5]
    # float32: the two middle neighbours are neighbouring float32 numbers, so their float64 mean is no float32
    a = np.float32(100.25)
    b = np.nextafter(a, np.float32(np.inf))
    v32 = np.full((9, 11), a, dtype=np.float32)
    v32[2:7, 3:8].flat[::2] = b  # 13 of the window's 25, the centre among them: 12 neighbours each of a and b
    v32[4, 5] = 500.0
    med32 = (np.float64(a) + np.float64(b)) * 0.5
    assert np.float64(np.float32(med32)) != med32
    out32, counts = DO.despike(v32, n_iter=1, replace="median")
    assert out32.dtype == np.float32 and out32[4, 5] == np.float32(med32) and out32[4, 5] in (a, b)


def test_a_pixel_with_too_few_neighbours_is_kept():
    v = np.full((7, 7), np.nan)
    v[3, 3] = 1000.0
    v[3, 4], v[2, 3], v[4, 4], v[3, 1] = 1.0, 2.0, 3.0, 2.5  # four neighbours within R = 2
    assert DO.despike(v, n_iter=1, min_neighbours=5)[1] == [0]
    out, counts = DO.despike(v, n_iter=1, min_neighbours=4)
    assert counts == [1] and np.isnan(out[3, 3])
    # the window is clipped at the image edge, not mirrored: a corner pixel of a 2 x 2 image has three neighbours
    c = np.array([[900.0, 1.0], [2.0, 3.0]])
    assert DO.despike(c, n_iter=1, min_neighbours=4)[1] == [0]
    assert DO.despike(c, n_iter=1, min_neighbours=3)[1] == [1]
    assert DO.despike(np.array([[5.0]]), n_iter=2, min_neighbours=1)[1] == [0, 0]  # no neighbour at all


def test_inf_is_no_neighbour_and_is_never_changed():
    rng = np.random.default_rng(1)
    v = 100.0 + rng.normal(0.0, 1.0, (9, 11))
    w = v.copy()
    w[4, 4], w[4, 6], w[0, 0] = np.inf, -np.inf, np.inf
    out, counts = DO.despike(w, n_iter=1, sign="both")
    hole = v.copy()
    hole[4, 4] = hole[4, 6] = hole[0, 0] = np.nan
    want, want_counts = DO.despike(hole, n_iter=1, sign="both")
    assert counts == want_counts
    assert out[4, 4] == np.inf and out[4, 6] == -np.inf and out[0, 0] == np.inf
    keep = np.isfinite(w)
    assert np.array_equal(out[keep], want[keep], equal_nan=True)


def test_a_second_run_on_a_result_that_flagged_nothing_changes_nothing():
    img, _, _ = DO.scene(np.float64)
    out, counts = DO.despike(img, n_iter=4)
    assert counts[0] > 0 and 0 in counts
    first_quiet = counts.index(0)
    assert all(c == 0 for c in counts[first_quiet:])
    again, counts2 = DO.despike(out, n_iter=2)
    assert counts2 == [0, 0] and np.array_equal(again, out, equal_nan=True)


def test_decisions_are_taken_on_the_pass_input():
    """Two spikes side by side: each sees the other as a neighbour in the same pass (Jacobi), whatever the scan order."""
    v = _flat((9, 12))
    v += np.random.default_rng(2).normal(0.0, 1.0, v.shape)
    v[4, 5], v[4, 6] = 5000.0, 4000.0
    out, counts = DO.despike(v, n_iter=1)
    out_t, counts_t = DO.despike(v.T.copy(), n_iter=1)
    assert counts == counts_t == [2] and np.array_equal(out, out_t.T, equal_nan=True)
    flipped, counts_f = DO.despike(v[::-1, ::-1].copy(), n_iter=1)
    assert counts_f == [2] and np.array_equal(out, flipped[::-1, ::-1], equal_nan=True)


# ---- the keyword ----------------------------------------------------------------------------------------------------------
def test_argument_forms():
    assert despike_params(None) is None
    assert despike_params(True) == DEFAULTS and despike_params(True) is not DEFAULTS
    assert DEFAULTS == dict(radius=2, nsigma=5.0, floor=0.0, min_neighbours=5, sign="positive", replace="nan", n_iter=2)
    assert DO.DEFAULTS == DEFAULTS
    assert despike_params(7) == {**DEFAULTS, "nsigma": 7.0} and isinstance(despike_params(7)["nsigma"], float)
    assert despike_params(np.float32(2.5))["nsigma"] == 2.5
    p = despike_params({"radius": 3, "min_neighbours": 48, "sign": "both", "replace": "median", "n_iter": 8, "floor": 2})
    assert p == dict(radius=3, nsigma=5.0, floor=2.0, min_neighbours=48, sign="both", replace="median", n_iter=8)
    assert despike_params({}) == DEFAULTS
    assert despike_params({"radius": np.int64(1), "min_neighbours": 8})["radius"] == 1
    assert despike_tag(None) == () and despike_tag(despike_params(True)) != despike_tag(despike_params(4.0))


@pytest.mark.parametrize("bad,match", [
    (False, "must be None"), ("median", "must be None"), ((5.0, 2), "must be None"), ([5.0], "must be None"),
    ({"sigma": 5.0}, "unknown key"), ({"radius": 2, "window": 5}, "unknown key"),
    ({"radius": 0}, "radius"), ({"radius": 4}, "radius"), ({"radius": 1.5}, "radius"), ({"radius": "2"}, "radius"),
    ({"radius": True}, "radius"),
    ({"n_iter": 0}, "n_iter"), ({"n_iter": 9}, "n_iter"), ({"n_iter": 2.5}, "n_iter"),
    ({"min_neighbours": 0}, "min_neighbours"), ({"min_neighbours": 25}, "min_neighbours"),
    ({"radius": 1, "min_neighbours": 9}, "min_neighbours"), ({"radius": 3, "min_neighbours": 49}, "min_neighbours"),
    (0, "nsigma"), (-1.0, "nsigma"), (float("nan"), "nsigma"), (float("inf"), "nsigma"), ({"nsigma": "5"}, "nsigma"),
    ({"nsigma": None}, "nsigma"),
    ({"floor": -1e-300}, "floor"), ({"floor": float("nan")}, "floor"), ({"floor": float("inf")}, "floor"),
    ({"floor": None}, "floor"),
    ({"sign": "negative"}, "sign"), ({"sign": 1}, "sign"), ({"replace": "mean"}, "replace"), ({"replace": 0}, "replace"),
])
def test_bad_arguments_raise(bad, match):
    with pytest.raises(ValueError, match=match):
        despike_params(bad, "despike_small")
    with pytest.raises(ValueError, match="despike_large"):
        despike_params(bad, "despike_large")


def test_limits_are_taken_on_their_good_side():
    for good in ({"radius": 1, "min_neighbours": 8}, {"radius": 3, "min_neighbours": 48}, {"min_neighbours": 24},
                 {"n_iter": 1}, {"n_iter": 8}, {"floor": 0.0}, {"nsigma": 5e-324}, {"min_neighbours": 1}):
        assert despike_params(good) == {**DEFAULTS, **good}


# ---- the classes ----------------------------------------------------------------------------------------------------------
def _alignment(**kw):
    from euispice_coreg_amd.hdrshift import Alignment
    return Alignment("no_such_large.fits", "no_such_small.fits", [0.0], [0.0], None, None, None, **kw)


def test_alignment_checks_the_keywords_before_anything_is_loaded():
    A = _alignment()
    assert A.despike_small is None and A.despike_large is None and A.last_despiked is None
    A = _alignment(despike_small=True, despike_large={"radius": 1, "min_neighbours": 3})
    assert A.despike_small == DEFAULTS and A.despike_large["radius"] == 1
    with pytest.raises(ValueError, match="despike_small"):
        _alignment(despike_small={"radius": 5})
    with pytest.raises(ValueError, match="despike_large.*unknown key"):
        _alignment(despike_large={"sigma": 3})
    with pytest.raises(ValueError, match="despike_large"):
        _alignment(despike_large="yes")


def test_the_tag_of_a_prepared_reference_names_the_parameters():
    def tagged(**kw):
        C = _alignment(**kw)
        C.lonlims, C.latlims, C.shape, C.order = (0, 1), (0, 1), (4, 4), 2
        C._reference_tag = lambda frame, *what: (frame,) + tuple(tuple(np.ravel(w).tolist()) for w in what)
        return C._carrington_tag(1.004, None)
    plain = tagged()
    assert tagged(despike_small=True) == plain  # (the image to align is no part of the reference)
    a, b = tagged(despike_large=True), tagged(despike_large=4.0)
    assert a != plain and a != b and a[:len(plain)] == plain and len(a) == len(plain) + 1
    assert tagged(despike_large=5.0) == a
    # an in-memory reference has no tag, with or without the keyword
    C = _alignment(despike_large=True)
    C.lonlims, C.latlims, C.shape, C.order = (0, 1), (0, 1), (4, 4), 2
    C._reference_tag = lambda frame, *what: None
    assert C._carrington_tag(1.004, None) is None


def test_the_other_classes_take_forward_and_check_the_keywords(tmp_path):
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    from euispice_coreg_amd.jitter_correction import jitter_correction as J
    S = AlignmentSpice("no_such_large.fits", "no_such_small.fits", [0.0], [0.0], despike_small=4.0,
                       despike_large={"sign": "both"})
    assert S.despike_small["nsigma"] == 4.0 and S.despike_large["sign"] == "both"
    with pytest.raises(ValueError, match="despike_small"):
        AlignmentSpice("no_such_large.fits", "no_such_small.fits", [0.0], [0.0], despike_small={"n_iter": 0})
    for fn in (J.jitter_correction_imagers, J._align_hrieuv_with_hrieuv):
        p = inspect.signature(fn).parameters
        assert p["despike_small"].default is None and p["despike_large"].default is None
    # refused before the first file is opened: the files do not exist
    with pytest.raises(ValueError, match="despike_large"):
        J.jitter_correction_imagers(["no_such_a.fits", "no_such_b.fits"], str(tmp_path / "out"), despike_large={"radius": 9})
    with pytest.raises(ValueError, match="despike_small"):
        J.jitter_correction_imagers(["no_such_a.fits", "no_such_b.fits"], str(tmp_path / "out"), despike_small="on")
    assert not (tmp_path / "out").exists()


def test_pxlshift_host_plan_holds_the_parameters(tmp_path):
    from tests import pxlshift_cases as Cs
    A, kw = Cs.make("a", tmp_path)
    assert A.last_despiked is None
    plan = A.host_plan(**kw)
    assert plan["despike_large"] is None and plan["despike_small"] is None and "bins_pending" not in plan
    plan = A.host_plan(**kw, despike_large=True, despike_small={"radius": 1, "min_neighbours": 4})
    assert plan["despike_large"] == DEFAULTS and plan["despike_small"]["min_neighbours"] == 4
    with pytest.raises(ValueError, match="despike_large"):
        A.host_plan(**kw, despike_large={"radius": 0})
    with pytest.raises(ValueError, match="despike_small.*unknown key"):
        A.host_plan(**kw, despike_small={"nsigmas": 3})
    # default bins are quantiles of the despiked images: pending until the GPU has made them; given edges are not
    plan = A.host_plan(**kw, method="mutual_information", despike_small=True)
    assert plan["bins"] is None and plan["bins_pending"] == 16
    plan = A.host_plan(**kw, method="mutual_information", despike_small=True, bins=([1.0, 2.0], [3.0]))
    assert "bins_pending" not in plan and len(plan["bins"][0]) == 2
    for fn in (A.find_best_parameters, A.find_local_shifts):
        p = inspect.signature(fn).parameters
        assert p["despike_large"].default is None and p["despike_small"].default is None


# ---- the seeded scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_seeded_scene(dtype):
    """96 x 128, truth = 200 + 150 sin(x/7) cos(y/9) + 80 exp(-((x-60)^2 + (y-40)^2)/50), image = poisson(truth), 150 pixels
    raised by uniform(300, 5000), the right-hand neighbours of the first 30 raised by 800, a 4 x 5 NaN block
    (default_rng(5); tests/despike_oracle.py: scene).  With the defaults the oracle must flag every raised pixel, at most
    0.1 % of the other finite pixels (12), and bring the masked Pearson coefficient against the truth from below 0.5 to
    above 0.95.  Measured with this generator's draws, both dtypes: 180 of 180 raised pixels flagged, 1 other pixel, counts
    per pass [181, 0], coefficient 0.2374 -> 0.9836."""
    img, truth, raised = DO.scene(dtype)
    assert img.dtype == dtype and img.shape == (96, 128) and raised.sum() == 180 and np.isnan(img).sum() == 20
    out, counts = DO.despike(img, **DEFAULTS)
    flagged = np.isfinite(img) & ~np.isfinite(out)
    others = int((flagged & ~raised).sum())
    before, after = DO.pearson(img, truth), DO.pearson(out, truth)
    print(f"[despike scene] {np.dtype(dtype).name}: {int((flagged & raised).sum())} of {int(raised.sum())} raised pixels "
          f"flagged, {others} others, counts {counts}, coefficient {before:.4f} -> {after:.4f}")
    assert out.dtype == dtype and sum(counts) == flagged.sum()
    assert (flagged & raised).sum() == raised.sum()
    assert others <= 12
    assert before < 0.5 and after > 0.95
    assert np.array_equal(out[~flagged], img[~flagged], equal_nan=True)  # nothing else is touched
