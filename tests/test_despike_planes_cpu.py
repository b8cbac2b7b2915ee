"""
CPU tests of the despiking of SPICE wavelength planes before they are summed (coreg_despike_sum_planes_be, the
`despike_planes=` keyword): the keyword's parser; the finding the feature rests on, in the numpy oracle -- hits of 0.4 x
the summed pixel value in the off-core planes of a SPICE-like window are out of the rule's reach in the summed image and
within it in the planes; and the plan (csrc/despike_planes_plan.hpp) on the host, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/native/despike_planes_rules.cpp, a program with its own main, run directly).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import despike_oracle as DO

HERE = os.path.dirname(os.path.abspath(__file__))
HIT_RULE = dict(DO.DEFAULTS, n_iter=1)
N_HITS = 60
HIT_PLANES = (1, 2, 5, 6)  # of 8: beside the line core (planes 3 and 4)


def hit_cube(fraction=0.4):
    """synthetic.make_spice_l2(nx=32, ny=96, nw=8) with N_HITS hits of `fraction` x the summed pixel value, each in one of
    HIT_PLANES at a pixel of its own, drawn with default_rng(5): (planes float32 [8, 96, 32], hit mask [96, 32], the
    4-D header, the reference image and its header)."""
    from euispice_coreg_amd import synthetic
    cube, h4, large, hl, _ = synthetic.make_spice_l2(nx=32, ny=96, nw=8)
    planes = np.array(cube[0], dtype=np.float32)
    rng = np.random.default_rng(5)
    ny, nx = planes.shape[1:]
    flat = rng.choice(ny * nx, size=N_HITS, replace=False)
    jj, ii = flat // nx, flat % nx
    kk = rng.choice(HIT_PLANES, size=N_HITS)
    summed = np.nansum(planes.astype(np.float64), axis=0)
    planes[kk, jj, ii] += (fraction * summed[jj, ii]).astype(np.float32)
    mask = np.zeros((ny, nx), dtype=bool)
    mask[jj, ii] = True
    return planes, mask, h4, large, hl


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_despike_planes_params_defaults_limits_and_unknown_keys():
    from euispice_coreg_amd.utils.despiking import DEFAULTS, despike_params, despike_planes_params
    assert despike_planes_params(None) is None
    want = dict(DEFAULTS, replace="median")
    assert despike_planes_params(True) == want
    assert despike_planes_params(4) == dict(want, nsigma=4.0) and despike_planes_params(3.5)["replace"] == "median"
    # a dict says what it wants: as despike_params
    assert despike_planes_params({}) == despike_params({}) == DEFAULTS
    assert despike_planes_params({"radius": 1, "n_iter": 1}) == dict(DEFAULTS, radius=1, n_iter=1)
    assert despike_planes_params({"replace": "median", "sign": "both"}) == dict(DEFAULTS, replace="median", sign="both")
    assert despike_params(True) == DEFAULTS  # (the other keywords keep their default)
    for bad in (False, "yes", [5.0], dict(radius=0), dict(radius=4), dict(n_iter=0), dict(n_iter=9), dict(nsigma=0.0),
                dict(nsigma=float("nan")), dict(nsigma=float("inf")), dict(floor=-1.0), dict(floor=float("nan")),
                dict(min_neighbours=0), dict(min_neighbours=25), dict(radius=1, min_neighbours=9), dict(sign="negative"),
                dict(replace="mean"), dict(radius=2.5), dict(window=5), 0, -3.0, float("nan")):
        with pytest.raises(ValueError) as e:
            despike_planes_params(bad)
        assert "despike_planes" in str(e.value), bad
    with pytest.raises(ValueError) as e:
        despike_planes_params(dict(window=5, radius=2))
    assert "window" in str(e.value)


def test_the_classes_refuse_a_bad_keyword_before_anything_is_loaded():
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster, AlignmentSpice
    with pytest.raises(ValueError):
        AlignmentSpice("no_such_large.fits", "no_such_L2.fits", despike_planes=dict(radius=9))
    with pytest.raises(ValueError):
        AlignementSpiceIterativeContextRaster([], "no_such_L2.fits", None, None, None, None, None, None,
                                              despike_planes="yes")
    A = AlignmentSpice("no_such_large.fits", "no_such_L2.fits", despike_planes=3)
    assert A.despike_planes["replace"] == "median" and A.despike_planes["nsigma"] == 3.0
    assert A.last_despiked_planes is None and A.despiked_plane_events is None
    assert AlignmentSpice("no_such_large.fits", "no_such_L2.fits").despike_planes is None


# ---- what it is for -----------------------------------------------------------------------------------------------------
def test_hits_in_a_plane_are_out_of_reach_after_the_sum():
    """The rule with its defaults and one pass finds at most 10 of the 60 hits in the summed image and at least 50 of them
    plane by plane; the plane oracle's event map says the same."""
    from tests import despike_planes_oracle as PO
    planes, mask, *_ = hit_cube()
    assert int(mask.sum()) == N_HITS
    summed = np.nansum(planes.astype(np.float64), axis=0)
    after, _ = DO.despike(summed, **HIT_RULE)
    found_after = int((np.isnan(after) & mask).sum())
    found_before = np.zeros(mask.shape, dtype=bool)
    for plane in planes:
        out, _ = DO.despike(plane, **HIT_RULE)
        found_before |= np.isnan(out)
    _, events, counts = PO.despike_sum_planes(planes, **HIT_RULE)
    print(f"[despike planes] hits found: {found_after} of {N_HITS} after the sum, {int((found_before & mask).sum())} plane by plane")
    assert found_after <= 10
    assert int((found_before & mask).sum()) >= 50
    assert np.array_equal(events > 0, found_before) and int(events.sum()) == sum(counts)


# ---- the plan on the host -----------------------------------------------------------------------------------------------
def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "despike_planes_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: despike planes rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_despike_planes_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "despike_planes_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    assert "warning" not in cc.stderr, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_despike_planes_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "despike_planes_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
