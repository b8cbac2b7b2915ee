"""
Seeded fuzz of the five sweep kernel families of pxlshift -- the Pearson and the `residus_masked` passes of
k_pixels_sweep and k_pixels_sweep_tiles, the weighted passes of k_pixels_lct, k_pixels_mi with 256 and 512 threads, tiled
and not -- over the cases of tests/pxlshift_fuzz_cases.py: lag lists as the planner's run rule can meet them (unsorted,
with duplicates, strides and lengths at which a run ends), image widths and pixel counts at the kernels' own edges,
NaN rows and columns, +-Inf, pixels <= 0, weight tables with zeros (tests/test_pxlshift_fuzz_cpu.py asserts that the seed
list walks every one of them).

Per seed ten calls through the public API -- `find_best_parameters` and `find_local_shifts` with disjoint tiles and with
a step, each with the three methods, and `find_local_shifts` with a step and weight tables -- against
tests/pxlshift_windows_oracle.py run on the device's own planes and box (`A._rotated(k)`, `A._large_box()`; the box is
compared bit for bit with `pxlshift_oracle.sub_resolution` cut to it, the unrotated planes with the small image):

  * counts, finite-term counts and histogram counts exactly; the same NaN pattern (an overlap that holds an Inf is NaN for
    the two coefficients, an Inf is dropped by `residus_masked` and binned by mutual information);
  * the bounds of tests/test_gpu_pxlshift_windows.py: the Pearson coefficient, weighted or not, 2^-23 |want| + 1e-12;
    `residus_masked` 1e-10 relative; mutual information 1e-11 absolute; weight sums 1e-12 relative;
  * over all Pearson entries of a seed at most 1 in 100 (one, when there are fewer than 100) beyond the tight bound of
    1e-12 (planes rotated by an angle != 0: 1e-10), the cap of tests/test_gpu_pxlshift.py: the float32 allowance is there
    for two numerators on either side of a rounding boundary and must not hide a wrong one
    (tests/test_pxlshift_fuzz_cpu.py holds the oracle itself, against a longdouble restatement, to the same cap);
  * the same best entry per window, up to the tie rule of tests/test_gpu_pxlshift_windows.py::_check;
  * slot and group independence, bit for bit: the same ten calls with `lag_dx` and `lag_dy` replaced by their sorted
    unique values give, at the position of every lag (every duplicate included), the same bits, counts and weight sums;
    equal rotation lags give equal planes of the cube.

Measured on one MI355X over the 35 seeds (`test_summary` prints the figures of a run): the coefficient, weighted or not,
4.4e-16 absolute (5.7e-16 relative); `residus_masked` 3.8e-16 relative; mutual information 1.8e-15 absolute; weight sums
5.9e-16 relative; 0 of 16 277 finite Pearson entries beyond the tight bound.  The whole file takes under 2 s.

Each of these changes to the library, tried one at a time, fails `test_seed` here (at the exact comparison of the counts,
or the NaN pattern): the run builder without its `lo = min(lo, v)` update, and `col_off` taken from the run's first entry
in place of its smallest (the ten seeds with a run whose minimum is not its first entry); `dc = step % 16` in the walk
of k_pixels_mi (23 seeds); the finite test in place of `a == a` in the Pearson pass (the nine seeds with an Inf in the
small image).
"""
import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels

from . import pxlshift_fuzz_cases as F
from . import pxlshift_oracle as O
from . import pxlshift_windows_oracle as Wd

pytestmark = pytest.mark.gpu

MI = "mutual_information"
METHODS = ("correlation", "residus_masked", MI)
KEYS = {"correlation": ("corr", "count"), "residus_masked": ("masked", "finite_terms"), MI: ("mi", "mi_count")}
KINDS = ("whole", "tiles", "windows")  # (a), (b), (c); (d) is ("apodized", "correlation")
worst = {}


def same_bits(a, b):
    """Equal shapes and equal bits, any two NaNs counting as equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _local(A, kw, method="correlation", **more):
    """(corr, counts, weight sums or None) of a `find_local_shifts` call.  A field without one valid window -- every entry
    NaN, as for the coefficient of a 1 x 1 image -- raises after the sweep has run: the cubes of the same plan are then read
    through the handle."""
    try:
        Fd = A.find_local_shifts(**kw, method=method, sub_lag=False, min_fill=0.0, **more)
        return Fd.corr, Fd.n_samples, Fd.weight_sums
    except ValueError as e:
        if "no valid tile" not in str(e):
            raise
    plan, hnd = A._last_plan, _lib.shared_handle(-1)
    corr = hnd.pixels_sweep_tiles(plan, plan["method_code"])
    assert not np.isfinite(corr).any()
    weights = None if plan["window"] is None else hnd.pixels_last_tile_weights(corr.shape)
    return corr, hnd.pixels_last_tile_counts(corr.shape), weights


def run(A, c, kw):
    """{(kind, method): (corr, counts, weight sums or None)} of the ten calls, every cube [n_ty][n_tx][n_dx][n_dy][n_rot]."""
    out = {}
    for m in METHODS:
        more = dict(bins=c["bins"]) if m == MI else {}
        corr = A.find_best_parameters(**kw, method=m, **more)
        out["whole", m] = (corr[None, None], A.last_counts[None, None], None)
        out["tiles", m] = _local(A, kw, m, tile_shape=c["tile_shape"], **more)
        out["windows", m] = _local(A, kw, m, tile_shape=c["tile_shape"], tile_step=c["tile_step"], **more)
    out["apodized", "correlation"] = _local(A, kw, tile_shape=c["tile_shape"], tile_step=c["tile_step"],
                                            apodization=c["window"])
    return out


def _bound(want, method):
    if method == "correlation":
        return 2.0 ** -23 * np.abs(want) + 1e-12
    return 1e-10 * np.abs(want) if method == "residus_masked" else np.full(want.shape, 1e-11)


def check(got, want, method, label, tight, tally):
    """A call's cubes against the oracle's: the NaN pattern, the bound of the method, the best entry per window with the
    tie rule (another best entry passes when the oracle's own scores of the two lie within twice the bound).  tight
    [n_rot]: the tight bound of every plane; tally: [entries beyond it, entries] of the seed's Pearson entries."""
    assert got.shape == want.shape and got.dtype == np.float64, label
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    fin = np.isfinite(want)
    d = np.abs(got - want)
    bound = _bound(want, method)
    with np.errstate(all="ignore"):
        rel = d[fin] / np.abs(want[fin])
    m = (float(d[fin].max()), float(np.nanmax(rel)) if np.isfinite(rel).any() else 0.0) if fin.any() else (0.0, 0.0)
    worst[method] = tuple(max(a, b) for a, b in zip(worst.get(method, (0.0, 0.0)), m))
    print(label, method, "max |diff|", m[0], "max relative", m[1], "finite entries", int(fin.sum()), "of", fin.size)
    assert np.all(d[fin] <= bound[fin]), label
    if method == "correlation":
        tally[0] += int((d > np.broadcast_to(tight, d.shape))[fin].sum())
        tally[1] += int(fin.sum())
    arg = np.nanargmin if method == "residus_masked" else np.nanargmax
    for ty in range(want.shape[0]):
        for tx in range(want.shape[1]):
            if np.isfinite(want[ty, tx]).any():
                g, w = arg(got[ty, tx]), arg(want[ty, tx])
                if g != w:
                    wt = want[ty, tx].ravel()
                    assert abs(wt[g] - wt[w]) <= 2 * bound[ty, tx].ravel()[w], (label, ty, tx)


def check_weights(got, want, label):
    assert got.shape == want.shape and np.isfinite(got).all(), label
    with np.errstate(all="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / want, np.abs(got - want))
    worst["weights"] = max(worst.get("weights", 0.0), float(rel.max()))
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), label


@pytest.mark.parametrize("seed", F.SEEDS)
def test_seed(seed):
    c = F.case(seed)
    A = AlignmentPixels((c["large"], dict(c["hdr_large"])), 0, (c["small"], dict(c["hdr_small"])), 0)
    kw = dict(lag_dx=c["lag_dx"], lag_dy=c["lag_dy"], lag_drot=c["lag_drot"])
    small, (h, w) = c["small"], c["small"].shape
    ts, step = c["tile_shape"], c["tile_step"]
    label = f"seed {seed} {h} x {w} {c['kinds']['dx']}/{c['kinds']['dy']}/{c['kinds']['drot']}"
    got = run(A, c, kw)

    # the device's own images: the box and the unrotated planes are the oracle's, bit for bit
    plan = A.host_plan(**kw, tile_shape=ts, tile_step=step, apodization=c["window"])
    plan["bins"] = A.host_plan(**kw, method=MI, bins=c["bins"])["bins"]
    planes, box = [A._rotated(k) for k in range(len(plan["lag_drot"]))], A._large_box()
    dx, dy, l = plan["lag_dx"], plan["lag_dy"], plan["slc_small_ref"]
    sub = O.sub_resolution(c["large"], plan["ratio_res_1"], plan["ratio_res_2"])
    assert same_bits(box, sub[l[0] + dy.min():l[0] + dy.max() + h, l[1] + dx.min():l[1] + dx.max() + w]), label
    for k, a in enumerate(plan["lag_drot"]):
        assert a != 0.0 or same_bits(planes[k], small), label
    tight = np.where(plan["lag_drot"] != 0.0, 1e-10, 1e-12)

    # (a) one window of the whole image, (b) disjoint tiles, (c) windows at a step, (d) the same with the weight tables
    oracle = {"whole": Wd.scores(None, small, plan, (h, w), None, planes=planes, box=box, mi=True),
              "tiles": Wd.scores(None, small, plan, ts, None, planes=planes, box=box, mi=True),
              "windows": Wd.scores(None, small, plan, ts, step, window=plan["window"], planes=planes, box=box, mi=True)}
    tally = [0, 0]
    for kind in KINDS:
        for m in METHODS:
            corr, counts, weights = got[kind, m]
            key, nkey = KEYS[m]
            assert weights is None and counts.dtype == np.float64
            assert np.array_equal(counts, oracle[kind][nkey]), (label, kind, m)
            check(corr, oracle[kind][key], m, f"{label} {kind}", tight, tally)
    corr, counts, weights = got["apodized", "correlation"]
    assert np.array_equal(counts, oracle["windows"]["count"]), label
    check(corr, oracle["windows"]["wcorr"], "correlation", f"{label} apodized", tight, tally)
    check_weights(weights, oracle["windows"]["weight"], label)
    print(label, "Pearson entries beyond the tight bound:", tally[0], "of", tally[1])
    assert tally[0] <= max(1, tally[1] // 100), (label, tally)
    worst["beyond"] = tuple(a + b for a, b in zip(worst.get("beyond", (0, 0)), tally))

    # slot and group independence: the sorted unique lists give every lag the same bits wherever it stood
    ux, uy = np.unique(dx), np.unique(dy)
    px, py = np.searchsorted(ux, dx), np.searchsorted(uy, dy)
    again = run(A, c, dict(kw, lag_dx=ux, lag_dy=uy))
    rot = plan["lag_drot"]
    for at, cubes in got.items():
        for first, second in zip(cubes, again[at]):
            assert (first is None) == (second is None)
            if first is not None:
                assert second.shape[2:4] == (len(ux), len(uy)), (label, at)
                assert same_bits(first, second[:, :, px][:, :, :, py]), (label, at)
                for k in range(1, len(rot)):
                    j = int(np.flatnonzero(rot == rot[k])[0])
                    assert j == k or same_bits(first[..., k], first[..., j]), (label, at, k)


def test_summary():
    """The largest differences met over the seeds (run after them; prints only)."""
    for key in METHODS:
        if key in worst:
            print(key, "max |diff|", worst[key][0], "max relative", worst[key][1])
    print("weight sums: max relative", worst.get("weights"))
    print("Pearson entries beyond the tight bound: %d of %d" % worst.get("beyond", (0, 0)))
