"""
Packed lag patches and the wave -> (point-group, lag-wave) mapping of k_sweep (csrc/lag_plan.hpp, kernels_sweep.hpp), on
an MI355X: lag planes whose batches have one, two, three and four live lag-waves and a ragged last wave, each against

  * the CPU oracle, at the tolerance the parity tests state for the frame (Carrington 1e-10, both methods, absolute;
    helioprojective 1e-7, float32 samples on both sides), and
  * the same sweep with `patch_w` forced, which plans the single rectangle of before: 1e-12 absolute (helioprojective
    1e-10), the project's bounds for two partitions of one sweep -- only the grouping of the sums may differ.

Which batches these planes give is asserted on the host (tests/native/lag_plan_rules.cpp, images this small: every window
fits): 8 x 8 one live wave, 8 x 16 two, 9 x 15, 16 x 12 and 33 x 17 (three patches of 11 x 17) three, 20 x 20 one of four
and one of three.  For the planes that are one patch the forced plan is the same rectangle: there the oracle is the check
of the wave mapping, and the comparison with the forced plan is exact.

Also a pair of lag slices cut in mid-row and a two-share point-sharded sweep, equal to the full map at the same bounds.
Grids of 64 x 56 points and images of 96 pixels: every case takes a second or two.
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPE = (64, 56)
# 8 x 8: one live wave; 8 x 16: two; 9 x 15 = 135: two full waves and 7 lags; 16 x 12: three full waves; 20 x 20 and
# 33 x 17: several batches, full and short ones
PLANES = [(8, 8), (8, 16), (9, 15), (16, 12), (20, 20), (33, 17)]


def _lags(n1, n2, step=2.0):
    return (17.0 + step * (np.arange(n1) - n1 // 2), -9.0 + step * (np.arange(n2) - n2 // 2), None, None, None)


_scene = {}


def scene(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _scene:
        _scene[key] = H.scene(**kw)
    return _scene[key]


class forced_single_rectangle:
    """`patch_w` = 256: one patch shape of any width, the plan of before."""

    def __init__(self, h):
        self.h = h

    def __enter__(self):
        self.h.set_option("patch_w", 256)

    def __exit__(self, *exc):
        self.h.set_option("patch_w", 0)


def _maxdiff(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b))) if np.isfinite(a).any() else 0.0


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_carrington_planes_vs_oracle_and_the_single_rectangle(gpu_handle, plane):
    """The default scene: 0.5 % NaN pixels in the image to align."""
    small, hs, large, hl, _ = scene()
    assert np.isnan(small).any()
    lags = _lags(*plane)
    want = H.oracle_carrington(small, hs, large, hl, lags, SHAPE)
    got = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, SHAPE)
    with forced_single_rectangle(gpu_handle):
        old = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, SHAPE, prepare=False)
    print(f"{plane}: max|d| oracle {_maxdiff(got, want):.3e}, single rectangle {_maxdiff(got, old):.3e}")
    H.assert_corr_close(got, want, 1e-10, f"carrington {plane}")
    assert _maxdiff(got, old) <= 1e-12


@pytest.mark.parametrize("plane", [(9, 15), (20, 20)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_carrington_residus_vs_oracle_and_the_single_rectangle(gpu_handle, plane):
    from euispice_coreg_amd import _lib
    from oracle import coreg_oracle as O
    small, hs, large, hl, _ = scene(nan_frac=0.0)
    lags = _lags(*plane)
    # a grid well inside the small field of view for every lag: the method gives a number only under full overlap
    lon, lat, shape = (243.0, 249.0), (2.0, 8.0), (40, 36)
    st = H.oracle_state(small, hs, large, hl, lags, shape=list(shape), lonlims=list(lon), latlims=list(lat),
                        solar_r=(1.004,))
    want = O.find_best_header_parameters(st, "carrington", method="residus")
    assert np.isfinite(want).all()
    grid = _lib.Grid(lon, lat, shape)
    ls = _lib.LagSet(*lags)
    gpu_handle.set_small(small)
    gpu_handle.prepare_reference_carrington(large, hl, grid, 1.004, 2)
    got = gpu_handle.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_RESIDUS)
    with forced_single_rectangle(gpu_handle):
        old = gpu_handle.sweep_carrington(hs, grid, 1.004, ls, method=_lib.METHOD_RESIDUS)
    print(f"residus {plane}: max|d| oracle {_maxdiff(got, want):.3e}, single rectangle {_maxdiff(got, old):.3e}, "
          f"max|want| {np.abs(want).max():.3e}")
    # (absolute bounds, on a statistic of about 8 here: an ulp of it is 9e-16)
    assert _maxdiff(got, want) <= 1e-10
    assert np.argmin(got) == np.argmin(want)
    assert _maxdiff(got, old) <= 1e-12


@pytest.mark.parametrize("order,plane", [(2, (9, 15)), (3, (16, 12))], ids=["order2-9x15", "order3-16x12"])
def test_helioprojective_vs_oracle_the_single_rectangle_slices_and_shares(gpu_handle, order, plane):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = scene(small_n=80, large_n=128)
    lags = _lags(*plane)
    ls = _lib.LagSet(*lags)
    want = H.oracle_helio(small, hs, large, hl, lags, order=order)
    got = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order)
    with forced_single_rectangle(gpu_handle):
        old = H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order, prepare=False)
    print(f"helio order {order} {plane}: max|d| oracle {_maxdiff(got, want):.3e}, single rectangle {_maxdiff(got, old):.3e}")
    H.assert_corr_close(got, want, 1e-7, f"helio order {order} {plane}")
    assert _maxdiff(got, old) <= 1e-10
    # two slices that meet in the middle of a CRVAL1 row
    cut = plane[1] * (plane[0] // 2) + plane[1] // 3
    parts = [H.gpu_helio(gpu_handle, small, hs, large, hl, lags, order=order, lag_begin=lo, lag_end=hi, prepare=False)
             for lo, hi in [(0, cut), (cut, ls.size)]]
    assert _maxdiff(np.concatenate(parts), got) <= 1e-10
    # two shares of the grid's points, added
    try:
        total = None
        for r in range(2):
            gpu_handle.set_point_shard(r, 2)
            gpu_handle.sweep_helioprojective(hs, hs, ls, order=order)
            s = gpu_handle.copy_sums()
            total = s if total is None else total + s
        shared = gpu_handle.finalize_sums(total, ls.size)
    finally:
        gpu_handle.set_point_shard(0, 1)
    assert _maxdiff(shared, got) <= 1e-10


def test_carrington_slices_and_point_shares_equal_the_full_map(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl, _ = scene()
    plane = (20, 20)
    lags = _lags(*plane)
    ls = _lib.LagSet(*lags)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, SHAPE)
    full = H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, SHAPE).ravel()
    # (one cut in mid-row, one that leaves a slice inside a single row)
    for cuts in [(0, 20 * 7 + 9, 400), (0, 20 * 11 + 2, 20 * 11 + 15, 400)]:
        parts = [H.gpu_carrington(gpu_handle, small, hs, large, hl, lags, SHAPE, lag_begin=lo, lag_end=hi, prepare=False)
                 for lo, hi in zip(cuts[:-1], cuts[1:])]
        d = _maxdiff(np.concatenate(parts), full)
        print(f"slices {cuts}: max|d| {d:.3e}")
        assert d <= 1e-12
    try:
        total = None
        for r in range(2):
            gpu_handle.set_point_shard(r, 2)
            assert np.isnan(gpu_handle.sweep_carrington(hs, grid, 1.004, ls)).all()
            s = gpu_handle.copy_sums()
            total = s if total is None else total + s
        shared = gpu_handle.finalize_sums(total, ls.size)
    finally:
        gpu_handle.set_point_shard(0, 1)
    d = _maxdiff(shared, full)
    print(f"two point shares: max|d| {d:.3e}")
    assert d <= 1e-12
