"""
CPU checks of the pxlshift fuzz cases (tests/pxlshift_fuzz_cases.py), no GPU:

  * coverage: over `SEEDS` every named lag-list kind, width, pixel count, tile width, bins kind and special pixel value
    occurs, and `groups_of` -- the planner's run rule restated -- reports a run of exactly 16, a run of 1 after a run of
    16, a run whose smallest lag is not its first entry, a run with a duplicate and a value in two runs.  A generator edit
    that drops an edge fails here;
  * every seed's `host_plan` succeeds for the three methods, with the lists as drawn and sorted-unique, and its tile
    grid is that of `pxlshift_windows_oracle.window_slices`;
  * the oracle against itself in higher precision: the Pearson coefficient, the weighted coefficient and
    `residus_masked` restated with their sums in np.longdouble and the same float32 rounding of the numerator, against
    `pxlshift_windows_oracle.scores` on every seed's stepped grid and whole image.  The GPU test
    (tests/test_gpu_pxlshift_fuzz.py) lets at most 1 Pearson entry in 100 of a seed (at most one when it has fewer than
    100) differ from the oracle by more than the tight bound of 1e-12: the rest of its bound, 2^-23 |corr|, is there for
    two numerators on either side of a float32 rounding boundary.  Here the same share is measured between two
    orderings of the oracle's own sums and held to the same cap, so a seed on which the oracle alone would spend the
    allowance is found here; `residus_masked` is held to its 1e-10 relative.
"""
import numpy as np
import pytest

from euispice_coreg_amd.pxlshift import AlignmentPixels

from . import pxlshift_fuzz_cases as F
from . import pxlshift_oracle as O
from . import pxlshift_windows_oracle as Wd

METHODS = ("correlation", "residus_masked", "mutual_information")
TIGHT = 1e-12


def obj(c):
    return AlignmentPixels((c["large"], dict(c["hdr_large"])), 0, (c["small"], dict(c["hdr_small"])), 0)


def lags(c, unique=False):
    dx, dy = (np.unique(c[k]) if unique else c[k] for k in ("lag_dx", "lag_dy"))
    return dict(lag_dx=dx, lag_dy=dy, lag_drot=c["lag_drot"])


def cap(n):
    """Entries of n that may exceed the tight bound: 1 in 100, one when there are fewer than 100."""
    return max(1, n // 100)


@pytest.fixture(scope="module")
def cases():
    return {s: F.case(s) for s in F.SEEDS}


# -------------------------------------------------------------------------------------------------------- coverage
def test_run_rule_by_hand():
    assert F.groups_of([5, 0, 15]) == [(0, 3, 0)]  # the minimum arrives second: one run of 16 columns
    assert F.groups_of([5, 0, 16]) == [(0, 2, 0), (2, 1, 16)]
    assert F.groups_of([5, 16, 0]) == [(0, 2, 5), (2, 1, 0)]
    assert F.groups_of(range(16)) == [(0, 16, 0)] and F.groups_of(range(17)) == [(0, 16, 0), (16, 1, 16)]
    assert F.groups_of(range(33)) == [(0, 16, 0), (16, 16, 16), (32, 1, 32)]
    assert F.groups_of(range(0, 16, 2)) == [(0, 8, 0)] and F.groups_of(range(0, 18, 2)) == [(0, 8, 0), (8, 1, 16)]
    assert F.groups_of([0, 15, 30]) == [(0, 2, 0), (2, 1, 30)] and F.groups_of([0, 16]) == [(0, 1, 0), (1, 1, 16)]
    assert F.groups_of([3, 3, 2, 3]) == [(0, 4, 2)] and F.groups_of(range(9, -8, -1)) == [(0, 16, -6), (16, 1, -7)]


def test_the_seed_list_walks_every_edge(cases):
    count = {}
    for s, c in cases.items():
        h, w = c["small"].shape
        assert h * w <= 2100 and len(c["lag_dx"]) * len(c["lag_dy"]) * len(c["lag_drot"]) <= F.MAX_LAGS
        assert np.array_equal(F.case(s)["small"], c["small"], equal_nan=True)  # the seed alone decides
        for m in F.marks(c):
            count[m] = count.get(m, 0) + 1
    need = F.required()
    for m in sorted(need | set(count), key=str):
        print(f"{'*' if m in need else ' '} {' '.join(str(v) for v in m):40s} {count.get(m, 0):3d}")
    assert not need - set(count), sorted(need - set(count), key=str)
    assert count[("ratio", "unequal_non_unit")] >= 3
    assert 30 <= len(F.SEEDS) <= 45 and len(set(F.SEEDS)) == len(F.SEEDS)


def test_the_bins_run_both_workgroup_sizes(cases):
    """csrc/host_pixels.hpp: 512 threads when 16 * na * nb * 4 bytes of histograms exceed 16384."""
    seen = set()
    for c in cases.values():
        es, el = obj(c).host_plan(**lags(c), method="mutual_information", bins=c["bins"])["bins"]
        na, nb = len(es) + 1, len(el) + 1
        seen.add(("wide" if 16 * na * nb * 4 > 16384 else "narrow", "na != nb" if na != nb else "na == nb"))
        seen.add((na, nb))
    print(sorted(seen, key=str))
    assert {("wide", "na != nb"), ("wide", "na == nb"), ("narrow", "na != nb"), ("narrow", "na == nb")} <= seen
    assert {(2, 2), (16, 16), (32, 32), (4, 32), (32, 16), (17, 16)} <= seen


# ------------------------------------------------------------------------------------------------------- the plans
def test_every_plan_succeeds(cases):
    for s, c in cases.items():
        A = obj(c)
        assert np.array_equal(A.data_small, c["small"], equal_nan=True)
        for unique in (False, True):
            for method in METHODS:
                kw = dict(bins=c["bins"]) if method == METHODS[2] else {}
                p = A.host_plan(**lags(c, unique), method=method, tile_shape=c["tile_shape"], tile_step=c["tile_step"], **kw)
                slices = Wd.window_slices(c["small"].shape, c["tile_shape"], c["tile_step"])
                assert p["tile_grid"] == (len(slices), len(slices[0])), s
                assert (p["ratio_res_1"], p["ratio_res_2"]) == c["kinds"]["ratio"]
            p = A.host_plan(**lags(c, unique), tile_shape=c["tile_shape"])
            slices = Wd.window_slices(c["small"].shape, c["tile_shape"])
            assert p["tile_grid"] == (len(slices), len(slices[0])), s
            p = A.host_plan(**lags(c, unique), tile_shape=c["tile_shape"], tile_step=c["tile_step"], apodization=c["window"])
            assert np.array_equal(p["window"][0], c["window"][0]) and np.array_equal(p["window"][1], c["window"][1])


# --------------------------------------------------------------------------- the oracle against itself, longdouble
def coefficient_ld(win, plane, wgt=None):
    """The (weighted) Pearson coefficient with its sums in np.longdouble, the numerator then rounded to float32."""
    a, b = plane.ravel(), win.ravel()
    keep = ~np.isnan(a) & ~np.isnan(b)
    w = np.ones(a.shape) if wgt is None else np.asarray(wgt, dtype=np.float64).ravel()
    a, b, w = a[keep].astype(np.longdouble), b[keep].astype(np.longdouble), w[keep].astype(np.longdouble)
    with np.errstate(all="ignore"):
        W = w.sum()
        if W == 0:
            return np.nan
        da, db = a - (w * a).sum() / W, b - (w * b).sum() / W
        num, va, vb = np.float32((w * da * db).sum()), (w * da * da).sum(), (w * db * db).sum()
        if va == 0 or vb == 0:
            return np.nan
        return float(np.longdouble(num) / np.sqrt(va * vb))


def masked_ld(win, plane):
    """np.std of the float64 terms (b - a) / sqrt(b) over isfinite(a) & isfinite(b), mean and squares in np.longdouble."""
    keep = np.isfinite(win) & np.isfinite(plane)
    with np.errstate(all="ignore"):
        d = ((win - plane) / np.sqrt(win))[keep].astype(np.longdouble)
        if not d.size:
            return np.nan
        return float(np.sqrt(((d - d.mean()) ** 2).sum() / d.size))


def test_the_oracle_against_itself_in_longdouble(cases):
    assert np.finfo(np.longdouble).nmant > 52, "np.longdouble is float64 here: nothing to compare"
    total, over, worst, seen = {}, {}, {}, set()
    for s, c in cases.items():
        plan = obj(c).host_plan(**lags(c), tile_shape=c["tile_shape"], tile_step=c["tile_step"], apodization=c["window"])
        small, (h, w), l = c["small"], c["small"].shape, plan["slc_small_ref"]
        dx, dy = plan["lag_dx"], plan["lag_dy"]
        sub = O.sub_resolution(c["large"], plan["ratio_res_1"], plan["ratio_res_2"])
        box = sub[l[0] + dy.min():l[0] + dy.max() + h, l[1] + dx.min():l[1] + dx.max() + w]
        planes = [O.rotate(small, a, "degree") for a in plan["lag_drot"]]
        for ts, step in ((c["tile_shape"], c["tile_step"]), ((h, w), None)):
            win_tables = plan["window"] if step is not None else (np.ones(h), np.ones(w))
            o = Wd.scores(None, small, plan, ts, step, window=win_tables, planes=planes, box=box)
            # what the special pixels are there for does happen: a poisoned residus_masked entry; an overlap with an Inf,
            # NaN for the coefficient while residus_masked drops the pixel; an Inf under weight 0, NaN all the same
            if np.any(o["poisoned"] > 0):
                seen.add("poisoned")
            if np.any(np.isnan(o["corr"]) & np.isfinite(o["masked"]) & (o["count"] > o["finite_terms"])):
                seen.add("inf_overlap")
            if step is not None and c["kinds"]["inf_under_zero_weight"]:
                assert np.isnan(o["wcorr"][0, :, :, :, plan["lag_drot"] == 0.0]).any(), s
                seen.add("inf_under_zero_weight")
            ld = {k: np.full(o["corr"].shape, np.nan) for k in ("corr", "wcorr", "masked")}
            for ty, row in enumerate(Wd.window_slices((h, w), ts, step)):
                for tx, (r, cc) in enumerate(row):
                    wgt = Wd.weights_of(*win_tables, (r.stop - r.start, cc.stop - cc.start))
                    for k, plane in enumerate(planes):
                        for i, vx in enumerate(dx):
                            for j, vy in enumerate(dy):
                                r0, c0 = int(vy - dy.min()), int(vx - dx.min())
                                wn, pl = box[r0:r0 + h, c0:c0 + w][r, cc], plane[r, cc]
                                at = (ty, tx, i, j, k)
                                ld["corr"][at] = coefficient_ld(wn, pl)
                                ld["wcorr"][at] = coefficient_ld(wn, pl, wgt)
                                ld["masked"][at] = masked_ld(wn, pl)
            for key in ld:
                got, want = o[key], ld[key]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (s, key)
                fin = np.isfinite(want)
                d = np.abs(got[fin] - want[fin])
                if key == "masked":
                    assert np.all(d <= 1e-10 * np.abs(want[fin])), (s, key)
                    d = d / np.where(want[fin] == 0, 1.0, np.abs(want[fin]))
                else:
                    assert np.all(d <= 2.0 ** -23 * np.abs(want[fin]) + TIGHT), (s, key)
                    n_over = int((d > TIGHT).sum())
                    assert n_over <= cap(d.size), (s, key, n_over, d.size)
                    over[key] = over.get(key, 0) + n_over
                total[key] = total.get(key, 0) + int(d.size)
                worst[key] = max(worst.get(key, 0.0), float(d.max()) if d.size else 0.0)
    assert seen == {"poisoned", "inf_overlap", "inf_under_zero_weight"}, seen
    for key in ("corr", "wcorr"):
        print(f"{key}: {over[key]} of {total[key]} finite entries beyond {TIGHT} (share {over[key] / total[key]:.2e}), "
              f"largest difference {worst[key]:.3e}")
    print(f"masked: {total['masked']} finite entries, largest relative difference {worst['masked']:.3e}")
