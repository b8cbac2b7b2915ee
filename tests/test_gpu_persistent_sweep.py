"""
k_sweep's persistent workgroups (kernels_sweep.hpp, launch_sweep): a launch has as many workgroups as the device holds at
a time, and each runs (group, batch) ITEMS one after another -- its first by its block index, the later ones by tickets
drawn from the queue of its XCD slot.  Which workgroup runs an item has no part in the item's arithmetic, so every case
is compared three ways:

  * with the CPU oracle at the project's bounds (1e-10 where every visit is interior, 1e-9 on the Carrington frame
    otherwise, 1e-7 on the helioprojective and plate-carree frames);
  * BITWISE with the same sweep under sweep_wgs >= the item count: one item per workgroup, the schedule before the change;
  * on the four tile-visit counters (coreg_last_visit_counts), which the workgroups add up over their items.

A small problem only walks the queues when the option "sweep_wgs" caps the workgroups of a launch: 8 is one workgroup per
queue, which then runs every item of its slot; 12 is no multiple of 8 (the grid is rounded up to 16) and gives every queue
two workgroups that draw tickets against each other.  The 96^2 scene of tests/test_gpu_visit_setup.py; 17 x 17 lags are
two batches, the second with 33 live lags: 31 padding lanes in its second lag-wave -- or none at all where the planner
cuts the plane otherwise -- and whole lag-waves of padding behind them.
"""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import CARR_RTOL, assert_masked
from tests.test_gpu_scalar_count import GRID, LAGS, N, PX

pytestmark = pytest.mark.gpu

ONE_ITEM_EACH = 1 << 20  # sweep_wgs at or above any item count
CAPS = (8, 12)
KINDS = ("visits", "lds", "interior", "all_finite")
SWEEP_DEFAULTS = {"n_groups": 0, "tile_w": 0, "taper_frac": -1, "sweep_wgs": 0}


def counts(h):
    vc = h.last_visit_counts()
    return tuple(int(vc[k]) for k in KINDS)


def bitwise(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def scene96(f32_exact):
    small, hs, large, hl, _ = H.scene(small_n=N, large_n=N, nan_frac=0.0, float32_exact=f32_exact)
    for a in (small, large):
        a.setflags(write=False)
    return small, hs, large, hl


def plane(n1, n2, step=0.25 * PX):  # (17 lags an axis span the +-2 pixels of LAGS: every visit stays interior)
    return (17.0 + step * (np.arange(n1) - n1 // 2), -9.0 + step * (np.arange(n2) - n2 // 2), None, None, None)


def with_options(h, options, run):
    try:
        for name, value in options.items():
            h.set_option(name, value)
        return run()
    finally:
        for name, value in SWEEP_DEFAULTS.items():
            h.set_option(name, value)


def three_ways(h, run, want, atol, what, options, caps=CAPS, close=H.assert_corr_close):
    """`run()` sweeps on h under its current options.  One item per workgroup first (held to the oracle), then every cap:
    bitwise the same map, the same counters.  atol None: the Carrington frame's rule, 1e-10 when every visit ran the
    interior loop, else 1e-9."""
    base = with_options(h, dict(options, sweep_wgs=ONE_ITEM_EACH), run)
    base_counts = counts(h)
    if atol is None:
        atol = 1e-10 if base_counts[2] == base_counts[0] else 1e-9
    print(f"\n[persistent] {what}: one item per workgroup, counters {base_counts}, "
          f"max|d| = {np.nanmax(np.abs(base - want)):.3e} (bound {atol:.0e})")
    close(base, want, atol, what)
    for cap in tuple(caps) + (0,):  # (0: the device's own residency -- at these sizes again one item each)
        got = with_options(h, dict(options, sweep_wgs=cap), run)
        got_counts = counts(h)
        print(f"[persistent] {what}: sweep_wgs {cap}, counters {got_counts}, bitwise {bitwise(got, base)}")
        assert bitwise(got, base), f"{what}: sweep_wgs={cap} changed the map"
        assert got_counts == base_counts, f"{what}: sweep_wgs={cap} counters {got_counts} != {base_counts}"
        close(got, want, atol, f"{what} sweep_wgs={cap}")
    return base, base_counts


def carrington_run(h, small, hs, large, hl, lags, grid, order, method=0):
    from euispice_coreg_amd import _lib
    g = _lib.Grid(grid["lonlims"], grid["latlims"], grid["shape"])
    ls = _lib.LagSet(*lags)
    h.set_small(np.array(small))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, order)
    return lambda: h.sweep_carrington(hs, g, 1.004, ls, order=order, method=method).reshape(ls.shape + (1,))


GRID128 = dict(GRID, shape=(128, 128))  # 16 tiles of 64 x 16 points on the inner window: every visit interior
LAGS2 = plane(17, 17)                   # 289 lags: two batches, the second ragged


# ---- 1. orders, methods, pixel types: two batches, three groups per queue ---------------------------------------------
@pytest.mark.parametrize("f32_exact", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_orders_methods_and_pixel_types(gpu_handle, order, f32_exact):
    from euispice_coreg_amd import _lib
    from oracle import coreg_oracle as O
    small, hs, large, hl = scene96(f32_exact)
    options = dict(n_groups=24, tile_w=64)  # 24 groups x 2 batches: 6 items per queue
    st = H.oracle_state(small, hs, large, hl, LAGS2, order=order, shape=list(GRID128["shape"]),
                        lonlims=list(GRID128["lonlims"]), latlims=list(GRID128["latlims"]), solar_r=(1.004,))
    for method, name in ((_lib.METHOD_CORRELATION, "correlation"), (_lib.METHOD_RESIDUS, "residus")):
        want = O.find_best_header_parameters(st, "carrington", method=name)
        run = carrington_run(gpu_handle, small, hs, large, hl, LAGS2, GRID128, order, method)
        # (plain residus: 1e-10 of max|want| and the argmin rule, as tests/test_gpu_sweep_variants.py holds it)
        close = H.assert_corr_close if name == "correlation" else assert_masked
        _, c = three_ways(gpu_handle, run, want, CARR_RTOL, f"o{order} {'f32' if f32_exact else 'f64'} {name}", options,
                          close=close)
        assert c[2] == c[0] > 0, c  # (every visit interior: the 1e-10 bound)
        assert np.isfinite(want).any()


def test_many_visits_per_item(gpu_handle):
    """The 256 x 256 grid of tests/test_gpu_visit_setup.py: 64 tiles in 8 shares, eight or nine visits an item, two
    batches: the workgroup of a queue runs both, the record read ahead and the parities of the visit buffers start
    afresh with the second."""
    small, hs, large, hl = scene96(True)
    grid = dict(GRID, shape=(256, 256))
    want = H.oracle_carrington(small, hs, large, hl, LAGS2, order=2, **grid)
    run = carrington_run(gpu_handle, small, hs, large, hl, LAGS2, grid, 2)
    _, c = three_ways(gpu_handle, run, want, 1e-10, "many visits", dict(n_groups=8, tile_w=64, taper_frac=0), caps=(8,))
    assert c[2] == c[0] >= 128, c


# ---- 2. items without a live visit, groups without a share -------------------------------------------------------------
def test_items_whose_every_visit_is_culled(gpu_handle):
    """Two clusters of lags 60 pixels apart on the grid that is wider than the image's field of view: a batch of the far
    cluster finds no sample in the tiles the near cluster covers and the other way round, so for many (group, batch)
    items every visit is culled -- the first one too, which under the once-per-item lag extents passes no barrier of
    its own -- next to items with live visits on the same workgroup."""
    small, hs, large, hl = scene96(True)
    c1 = np.concatenate([17.0 + PX * (np.arange(9) - 64.0), 17.0 + PX * (np.arange(9) - 4.0)])
    lags = (c1, -9.0 + PX * (np.arange(18) - 9.0), None, None, None)
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **V.BORDER_GRID)
    run = carrington_run(gpu_handle, small, hs, large, hl, lags, V.BORDER_GRID, 2)
    _, c = three_ways(gpu_handle, run, want, None, "culled items", dict(n_groups=24))
    assert 0 < c[0], c
    assert np.isfinite(want).any()


def test_groups_with_an_empty_share(gpu_handle):
    """16 x 16 grid points are 16 work units; 24 groups: at least eight have u_lo == u_hi, walk no list entry and go
    straight to the reduction (their slabs are zero)."""
    small, hs, large, hl = scene96(True)
    grid = dict(GRID, shape=(16, 16))
    want = H.oracle_carrington(small, hs, large, hl, LAGS2, order=2, **grid)
    run = carrington_run(gpu_handle, small, hs, large, hl, LAGS2, grid, 2)
    three_ways(gpu_handle, run, want, 1e-10, "empty shares", dict(n_groups=24))


# ---- 3. several k_sweep launches behind one k_tile_list: a stale queue would show --------------------------------------
def test_helioprojective_order2(gpu_handle):
    sc = V.scene("helio-series", True, "interior")
    small, hs, large, hl, lags = sc["small"], sc["hs"], sc["large"], sc["hl"], sc["lags"]
    want = H.oracle_helio(small, hs, large, hl, lags, order=2)
    h = gpu_handle
    H.gpu_helio(h, small, hs, large, hl, lags, order=2)  # (uploads and prepares)
    v = h.last_sweep_variant()
    assert v["order"] == 2 and v["mode"] in (V.HOMOGRAPHY, V.HOMOGRAPHY_SERIES), v
    three_ways(h, lambda: H.gpu_helio(h, small, hs, large, hl, lags, order=2, prepare=False), want, 1e-7,
               "helioprojective o2 (h_incr on)", dict(n_groups=16))


def test_plate_carree_launch_per_combination(gpu_handle):
    from euispice_coreg_amd import _lib, synthetic
    small, hs, large, hl, _ = synthetic.make_car_scene(small_shape=(70, 96), large_shape=(110, 150), crota=0.3, seed=5,
                                                       small_cdelt=(0.0111, 0.0093), nan_frac=0.0)
    lags = (np.array([0.0, 0.012, 0.02]), np.array([-0.015, -0.004]), [0.0, 0.0002], None, [-0.2, 0.0])
    want = H.oracle_helio(small.astype(np.float64), hs, large.astype(np.float64), hl, lags, parallelism=False,
                          unit_lag="deg")
    h = gpu_handle
    ls = _lib.LagSet(*lags)
    h.set_small(small)
    h.set_reference_on_grid(np.asarray(large, dtype=np.float32))
    three_ways(h, lambda: h.sweep_helioprojective(hl, hs, ls, order=2).reshape(ls.shape + (1,)), want, 1e-7,
               "plate carree, 4 combinations", dict(n_groups=16))
    assert h.last_stats()["n_sweep_launches"] >= 4


def test_five_d_carrington(gpu_handle):
    small, hs, large, hl = scene96(True)
    lags = (LAGS[0], LAGS[1], None, None, np.array([-0.3, 0.0, 0.3]))  # three CROTA combinations: three launches
    want = H.oracle_carrington(small, hs, large, hl, lags, order=2, **GRID128)
    run = carrington_run(gpu_handle, small, hs, large, hl, lags, GRID128, 2)
    three_ways(gpu_handle, run, want, None, "5-D, 3 combinations", dict(n_groups=24, tile_w=64))
    assert gpu_handle.last_stats()["n_sweep_launches"] >= 3


# ---- 4. the queue from call to call, and two handles at once -----------------------------------------------------------
def test_twice_on_one_handle_and_two_handles_on_two_streams():
    """Every handle has a stream and a queue of its own.  Two host threads sweep four times each on their handles, started
    together (the library call releases the interpreter lock), so launches of the two are in flight at once; each
    thread's second to fourth sweeps find the queue the sweep before left."""
    import threading
    from euispice_coreg_amd import _lib
    small, hs, large, hl = scene96(True)
    g = _lib.Grid(GRID128["lonlims"], GRID128["latlims"], GRID128["shape"])
    ls = _lib.LagSet(*LAGS2)
    handles = [_lib.CoregHandle(0) for _ in range(2)]
    outs, errors = [[], []], []
    try:
        for h in handles:
            h.set_small(np.array(small))
            h.prepare_reference_carrington(np.array(large), hl, g, 1.004, 2)
            for name, value in dict(n_groups=24, tile_w=64, sweep_wgs=8).items():
                h.set_option(name, value)
        first = handles[0].sweep_carrington(hs, g, 1.004, ls)
        start = threading.Barrier(2)

        def work(k):
            try:
                start.wait(timeout=30)
                for _ in range(4):
                    outs[k].append(handles[k].sweep_carrington(hs, g, 1.004, ls))
            except Exception as e:  # (reported by the main thread)
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(2):
            assert len(outs[k]) == 4 and all(bitwise(o, first) for o in outs[k]), k
        want = H.oracle_carrington(small, hs, large, hl, LAGS2, order=2, **GRID128)
        H.assert_corr_close(first.reshape(ls.shape + (1,)), want, 1e-10, "two handles")
    finally:
        for h in handles:
            h.close()


# ---- 5. point shards: a launch whose first group is not group 0 --------------------------------------------------------
def test_point_shards_against_the_unsharded_map(gpu_handle):
    from euispice_coreg_amd import _lib
    small, hs, large, hl = scene96(True)
    h = gpu_handle
    g = _lib.Grid(GRID128["lonlims"], GRID128["latlims"], GRID128["shape"])
    ls = _lib.LagSet(*LAGS2)
    h.set_small(np.array(small))
    h.prepare_reference_carrington(np.array(large), hl, g, 1.004, 2)
    whole = h.sweep_carrington(hs, g, 1.004, ls)

    def shared(cap):
        total, seen = None, []
        try:
            h.set_option("tile_w", 64)
            h.set_option("sweep_wgs", cap)
            for r in range(2):
                h.set_point_shard(r, 2)
                assert np.isnan(h.sweep_carrington(hs, g, 1.004, ls)).all()
                seen.append(counts(h))
                part = h.copy_sums()
                total = part if total is None else total + part
            return h.finalize_sums(total, ls.size), seen
        finally:
            h.set_point_shard(0, 1)
            for name, value in SWEEP_DEFAULTS.items():
                h.set_option(name, value)

    base, base_counts = shared(ONE_ITEM_EACH)
    assert np.nanmax(np.abs(base - whole)) <= 1e-10  # (tests/test_gpu_car.py's bound on shares against one GPU's map)
    for cap in CAPS:
        got, got_counts = shared(cap)
        assert bitwise(got, base) and got_counts == base_counts, (cap, got_counts, base_counts)
