"""
GPU tests of coreg_despike_sum_planes_be and the `despike_planes=` keyword against tests/despike_planes_oracle.py, the
contract in numpy.  The rule is selection, comparison and separately rounded float64 operations, and the sum a float64
accumulation in a fixed order, so every comparison with the oracle is an equality: np.array_equal(equal_nan=True) on the sum,
np.array_equal on the events, equal count lists.  The shapes are those at which a tiled window kernel goes wrong (the tile
is read from csrc/despike_plan.hpp); the oracle walks pixels in Python, so every test stays below about 40 000 pixel
evaluations (planes x pixels x passes).
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import despike_oracle as DO
from tests import despike_planes_oracle as PO
from tests import helpers as H
from tests.despike_cases import TILE_H, TILE_W, image, rule, stack
from tests.test_despike_planes_cpu import HIT_RULE, N_HITS, hit_cube

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 40), (40, 1), (5, 7), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 3, TILE_W + 5)]
BIG = SHAPES[-1]  # several tiles, ragged in both axes


def check(h, planes, what, index=None, **prm):
    """One call through the binding on the big-endian stack against the oracle on planes[index]; the oracle's counts."""
    index = np.arange(len(planes)) if index is None else np.asarray(index)
    want_sum, want_events, want_counts = PO.despike_sum_planes(planes[index], **prm)
    got_sum, got_events, got_counts = h.despike_sum_planes(PO.be(planes), index, prm)
    assert got_sum.dtype == np.float64 and got_events.dtype == np.int32 and got_sum.shape == planes.shape[1:]
    assert got_counts == want_counts, f"{what}: flagged {got_counts}, the oracle {want_counts}"
    assert np.array_equal(got_events, want_events), f"{what}: the event map differs"
    assert np.array_equal(got_sum, want_sum, equal_nan=True), f"{what}: the sum differs"
    assert int(got_events.sum()) == sum(got_counts)
    return want_counts


# ---- 1. the kernels against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_planes_against_the_oracle(gpu_handle, shape, dtype):
    """1, 3 and 6 planes with n_iter 1, 2, 3 (the fused pass alone; each buffer of the passes before it as its input) and
    R = 1, 2, 3, the pairing of R and n_iter turning with the shape so that all nine pairs occur; NaN and median
    replacement, sign = both and a floor."""
    shift = SHAPES.index(shape) + (dtype == np.float64)
    flagged = 0
    for i, (n, n_iter) in enumerate([(1, 1), (3, 2), (6, 3)]):
        R = 1 + (i + shift) % 3
        v = stack(n, shape, 3 + 5 * i + shift, dtype)
        flagged += sum(check(gpu_handle, v, f"{n}x{shape} R={R} n_iter={n_iter}", **rule(R, n_iter, shape)))
        if n == 3:
            for R2 in (1, 2, 3):
                flagged += sum(check(gpu_handle, v, f"{n}x{shape} R={R2} both/median/floor",
                                     **rule(R2, 2, shape, sign="both", replace="median", floor=0.75, nsigma=3.0)))
    if shape[0] * shape[1] >= 35:
        assert flagged > 0  # the cases decide both ways


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_iter", [1, 2, 3])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_every_radius_with_every_pass_count(gpu_handle, R, n_iter, dtype):
    v = stack(3, (TILE_H + 1, TILE_W + 1), 40 + 3 * R + n_iter, dtype)
    assert sum(check(gpu_handle, v, f"R={R} n_iter={n_iter}", **rule(R, n_iter, replace="median" if n_iter == 2 else "nan"))) > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_an_image_is_a_stack_of_one_plane(gpu_handle, R, dtype):
    """coreg_despike_small on a resident image and coreg_despike_sum_planes_be on the same pixels as a one-plane big-endian
    cube: the sum is the despiked image (a NaN a zero term), the counts per pass are equal, and the event map, which the
    resident image has none of, holds the number of passes in which the oracle flags the pixel."""
    h = gpu_handle
    shape = (TILE_H + 1, TILE_W + 1)
    v = image(shape, 60 + R, dtype)
    prm = rule(R, 2, shape, replace="median", sign="both")
    h.set_small(v)
    counts = h.despike_small(prm)
    got = h.get_small(v.shape, v.dtype)
    total, events, plane_counts = h.despike_sum_planes(PO.be(v[None]), [0], prm)
    assert np.array_equal(total, np.where(np.isnan(got), 0.0, got.astype(np.float64)))
    assert plane_counts == counts
    want_events = np.zeros(shape, dtype=np.int32)
    out = v
    for _ in range(prm["n_iter"]):
        new, n = DO.despike_pass(out, **{k: x for k, x in prm.items() if k != "n_iter"})
        flagged = ~((new == out) | (np.isnan(new) & np.isnan(out)))  # (a flag event changes the pixel: |d| > 0)
        assert int(flagged.sum()) == n
        want_events += flagged
        out = new
    assert want_events.any() and np.array_equal(events, want_events)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_holes_infinities_ties_and_a_constant_stack(gpu_handle, dtype):
    """A NaN block wider than the window in some planes only, a pixel that is NaN in every plane (sum 0), +Inf in one plane
    (sum +Inf), +Inf and -Inf at one pixel in two planes (sum NaN, as numpy gives), integer planes, a constant stack."""
    ny, nx = BIG
    v = stack(3, BIG, 17, dtype)
    v[0, ny // 4:ny // 4 + 8, nx // 4:nx // 4 + 9] = np.nan
    v[2, ny // 4 + 2:ny // 4 + 10, nx // 4:nx // 4 + 9] = np.nan
    v[:, 2, 3] = np.nan
    v[1, ny // 2, nx // 2] = np.inf
    v[0, ny - 2, 5] = np.inf
    v[2, ny - 2, 5] = -np.inf
    for R in (1, 3):
        check(gpu_handle, v, f"holes R={R}", **rule(R, 2, sign="both"))
    check(gpu_handle, v, "holes median", **rule(2, 1, replace="median"))
    got, events, _ = gpu_handle.despike_sum_planes(PO.be(v), [0, 1, 2], rule(2, 2))
    assert got[2, 3] == 0.0 and got[ny // 2, nx // 2] == np.inf and np.isnan(got[ny - 2, 5])
    assert events[2, 3] == 0 and events[ny // 2, nx // 2] == 0 and events[ny - 2, 5] == 0
    ints = stack(3, BIG, 19, dtype, "integers")
    ints[1, 5, :] = np.nan
    check(gpu_handle, ints, "integers", **rule(2, 2, sign="both", floor=0.5))
    check(gpu_handle, ints, "integers median", **rule(1, 2, replace="median", floor=0.5))
    assert check(gpu_handle, stack(3, BIG, 0, dtype, "constant"), "constant", **rule(2, 2, sign="both")) == [0, 0]


# ---- 2. addressing -----------------------------------------------------------------------------------------------------
def raw_call(h, cube_be, stride, H_, W_, index, prm, bitpix=None, n_sel=None, offset=0, fill=-7.0):
    """coreg_despike_sum_planes_be itself on `cube_be` (a big-endian array) from element `offset`: (return code, sum,
    events, counts), the outputs pre-filled so that a refused call can be seen to leave them alone."""
    from euispice_coreg_amd import _lib
    index = np.ascontiguousarray(index, dtype=np.int64)
    p = _lib.DespikeParams.of(prm)
    out = np.full((max(H_, 1), max(W_, 1)), fill, dtype=np.float64)
    events = np.full(out.shape, -7, dtype=np.int32)
    counts = (C.c_int64 * 8)(*([-7] * 8))
    item = cube_be.dtype.itemsize
    rc = h._lib.coreg_despike_sum_planes_be(h._h, cube_be.ctypes.data + offset * item, -8 * item if bitpix is None else bitpix,
                                            stride, H_, W_, index.ctypes.data, len(index) if n_sel is None else n_sel,
                                            C.byref(p), out.ctypes.data, events.ctypes.data, counts)
    return rc, out, events, list(counts)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plane_order_duplicates_rows_and_stride(gpu_handle, dtype):
    h = gpu_handle
    prm = rule(2, 2)
    cube = stack(5, (TILE_H + 9, TILE_W + 1), 23, dtype)
    # out of order, with a duplicate: the float64 sum depends on the order, the oracle takes the planes as listed
    check(h, cube, "index [3, 0, 3, 1]", index=[3, 0, 3, 1], **prm)
    a, _, _ = h.despike_sum_planes(PO.be(cube), [3, 0, 1], prm)
    b, _, _ = h.despike_sum_planes(PO.be(cube), [0, 1, 3], prm)
    assert np.allclose(a, b, rtol=1e-12, equal_nan=True)
    # a row range inside the taller cube: the result of the cut-out stack, the rows outside never neighbours
    r0, r1 = 4, TILE_H + 5
    cut = np.ascontiguousarray(cube[:, r0:r1])
    want = PO.despike_sum_planes(cut[[1, 2, 4]], **prm)
    got = h.despike_sum_planes(PO.be(cube), [1, 2, 4], prm, rows=(r0, r1))
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    spiky = cube.copy()
    spiky[:, r0 - 1] += 5000.0  # the row above and the row below the range: were they neighbours, medians would move
    spiky[:, r1] -= 5000.0
    again = h.despike_sum_planes(PO.be(spiky), [1, 2, 4], prm, rows=(r0, r1))
    assert np.array_equal(again[0], got[0], equal_nan=True) and np.array_equal(again[1], got[1]) and again[2] == got[2]
    # plane_stride above H x W, by the call itself: planes padded with poison
    ny, nx = cut.shape[1:]
    padded = np.full((5, ny * nx + 13), 1e30, dtype=dtype)
    padded[:, :ny * nx] = cut.reshape(5, -1)
    rc, out, events, counts = raw_call(h, PO.be(padded), ny * nx + 13, ny, nx, [1, 2, 4], prm)
    assert rc == 0 and np.array_equal(out, want[0], equal_nan=True) and np.array_equal(events, want[1])
    assert counts[:2] == want[2] and counts[2:] == [-7] * 6


def test_native_and_integer_input_and_no_plane(gpu_handle):
    h = gpu_handle
    prm = rule(1, 2, replace="median")
    v32 = stack(3, (TILE_H + 1, TILE_W + 1), 29, np.float32)
    want = PO.despike_sum_planes(v32, **prm)
    # native little-endian, as stored, a (data, header) pair, an array that is not C-contiguous: the same values
    for given in (v32, PO.be(v32), (v32, {"NAXIS": 3}), np.asfortranarray(v32), PO.be(v32)[:, :, ::-1][:, :, ::-1]):
        got = h.despike_sum_planes(given, [0, 1, 2], prm)
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    ints = stack(3, (TILE_H + 1, TILE_W + 1), 31, np.float64, "integers").astype(np.int16)
    want = PO.despike_sum_planes(ints.astype(np.float64), floor=0.5, **prm)
    got = h.despike_sum_planes(ints, [0, 1, 2], dict(prm, floor=0.5), rows=None)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and sum(want[2]) > 0
    v64 = stack(2, (5, 7), 37, np.float64)
    want = PO.despike_sum_planes(v64, **rule(1, 1, (5, 7)))
    got = h.despike_sum_planes(v64, [0, 1], rule(1, 1, (5, 7)))
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    # no plane: +0.0 everywhere, no events, zero counts
    for given in (v32, PO.be(v32)):
        s, e, c = h.despike_sum_planes(given, [], prm)
        assert s.shape == v32.shape[1:] and not s.any() and not np.signbit(s).any() and not e.any() and c == [0, 0]
    with pytest.raises(IndexError):
        h.despike_sum_planes(v32, [0, 3], prm)
    with pytest.raises(ValueError):
        h.despike_sum_planes(v32[0], [0], prm)


# ---- 3. invariants -----------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_nothing_resident_changes(gpu_handle):
    from euispice_coreg_amd import _lib
    from tests.test_gpu_despike import REF_RULE, SHAPE, image, spiked
    h = gpu_handle
    v = spiked(image((37, 45), 2, np.float32), 4)
    small, hs, large, hl, _ = H.scene(small_n=40, large_n=160)
    large = spiked(large, 23)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, SHAPE)

    def ref():
        h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        return h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64)
    planes = PO.be(stack(4, BIG, 41, np.float64))
    try:
        h.set_small(v)
        h.despike_small(rule(2, 2))
        small_before = h.get_small(v.shape, np.float32)
        h.pixels_set_large(v)
        h.pixels_set_small(v[::-1].copy())
        h.set_reference_despike(REF_RULE)
        ref_before, counts_before = ref(), h.last_reference_despike()
        assert counts_before[0] > 0
        first = h.despike_sum_planes(planes, [0, 1, 2, 3], rule(3, 3, sign="both"))
        again = h.despike_sum_planes(planes, [0, 1, 2, 3], rule(3, 3, sign="both"))
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
        assert sum(first[2]) > 0 and int(first[1].sum()) == sum(first[2])
        assert h.last_reference_despike() == counts_before
        assert np.array_equal(h.get_small(v.shape, np.float32), small_before, equal_nan=True)
        assert np.array_equal(h.pixels_get_image("large", v.shape), v.astype(np.float64), equal_nan=True)
        assert np.array_equal(h.pixels_get_image("small", v.shape), v[::-1].astype(np.float64), equal_nan=True)
        assert np.array_equal(ref(), ref_before, equal_nan=True) and h.last_reference_despike() == counts_before
    finally:
        h.set_reference_despike(None)
    with _lib.CoregHandle(0) as fresh:  # no image at all: the call needs none
        with pytest.raises(_lib.CoregError) as e:
            fresh.despike_sum_planes_last_ms()
        assert e.value.code == _lib.COREG_ESTATE
        got = fresh.despike_sum_planes(planes, [0, 1, 2, 3], rule(3, 3, sign="both"))
        assert fresh.despike_sum_planes_last_ms() > 0.0
        assert got[0].tobytes() == first[0].tobytes() and got[2] == first[2]


def test_the_last_pass_without_its_second_window(gpu_handle):
    """Option "despike_planes_overlap" 0 (what the overlap is timed against): the same bits."""
    h = gpu_handle
    planes = PO.be(stack(4, BIG, 43, np.float32))
    want = h.despike_sum_planes(planes, [0, 1, 2, 3], rule(2, 2))
    h.set_option("despike_planes_overlap", 0)
    try:
        got = h.despike_sum_planes(planes, [0, 1, 2, 3], rule(2, 2))
        check(h, stack(3, (TILE_H + 1, TILE_W + 1), 45, np.float64), "no overlap", **rule(3, 1))
    finally:
        h.set_option("despike_planes_overlap", 1)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


def test_multi_handle_runs_it_on_its_first_device(gpu_handle, monkeypatch):
    from euispice_coreg_amd import _lib
    monkeypatch.setenv("COREG_VIRTUAL_DEVICES", "2")
    planes = PO.be(stack(3, BIG, 47, np.float32))
    want = gpu_handle.despike_sum_planes(planes, [2, 0, 1], rule(2, 2), rows=(1, BIG[0] - 2))
    with _lib.MultiHandle() as mh:
        got = mh.despike_sum_planes(planes, [2, 0, 1], rule(2, 2), rows=(1, BIG[0] - 2))
        with pytest.raises(_lib.CoregError) as e:
            mh.despike_sum_planes(planes, [0], dict(radius=7))
        assert e.value.code == _lib.COREG_EINVAL
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
# (tests/test_gpu_despike.py: BAD_RULES, restated)
BAD_RULES = [dict(radius=0), dict(radius=4), dict(n_iter=0), dict(n_iter=9), dict(nsigma=0.0), dict(nsigma=-1.0),
             dict(nsigma=float("nan")), dict(nsigma=float("inf")), dict(floor=-1.0), dict(floor=float("nan")),
             dict(floor=float("inf")), dict(min_neighbours=0), dict(min_neighbours=25), dict(radius=1, min_neighbours=9),
             dict(radius=3, min_neighbours=49), dict(sign=2), dict(sign=-1), dict(replace=2), dict(replace=-1)]


def test_refusals_by_error_code_and_outputs_untouched(gpu_handle):
    from euispice_coreg_amd import _lib
    from tests.test_gpu_despike import BAD_RULES as THEIRS
    assert repr(BAD_RULES) == repr(THEIRS)
    h = gpu_handle
    ny, nx = 9, 11
    v = PO.be(stack(3, (ny, nx), 51, np.float32))
    good = rule(2, 2)

    def refused(rc, out, events, counts, what):
        assert rc == _lib.COREG_EINVAL, what
        assert (out == -7.0).all() and (events == -7).all() and counts == [-7] * 8, what
        assert h._lib.coreg_last_error(h._h), what
    rc, out, events, counts = raw_call(h, v, ny * nx, ny, nx, [0, 1, 2], good)
    assert rc == 0 and not (out == -7.0).any() and counts[2:] == [-7] * 6
    for bad in BAD_RULES:
        refused(*raw_call(h, v, ny * nx, ny, nx, [0, 1, 2], bad), bad)
        with pytest.raises(_lib.CoregError) as e:
            h.despike_sum_planes(v, [0, 1, 2], bad)
        assert e.value.code == _lib.COREG_EINVAL, bad
    for bitpix in (32, 16, 8, 64, 0, -16):
        refused(*raw_call(h, v, ny * nx, ny, nx, [0, 1, 2], good, bitpix=bitpix), f"BITPIX {bitpix}")
    refused(*raw_call(h, v, ny * nx - 1, ny, nx, [0, 1, 2], good), "a stride below H x W")
    refused(*raw_call(h, v, ny * nx, 0, nx, [0, 1, 2], good), "no row")
    refused(*raw_call(h, v, ny * nx, ny, 0, [0, 1, 2], good), "no column")
    refused(*raw_call(h, v, ny * nx, ny, nx, np.zeros(4097, dtype=np.int64), good), "n_sel above the cap")
    refused(*raw_call(h, v, ny * nx, ny, nx, [0, 1, 2], good, n_sel=-1), "n_sel below zero")
    refused(*raw_call(h, v, ny * nx, ny, nx, [0, -1, 2], good), "a negative plane index")
    p = _lib.DespikeParams.of(good)
    idx = np.arange(3, dtype=np.int64)
    out = np.full((ny, nx), -7.0)
    fn = h._lib.coreg_despike_sum_planes_be
    assert fn(h._h, None, -32, ny * nx, ny, nx, idx.ctypes.data, 3, C.byref(p), out.ctypes.data, None, None) == _lib.COREG_EINVAL
    assert fn(h._h, v.ctypes.data, -32, ny * nx, ny, nx, None, 3, C.byref(p), out.ctypes.data, None, None) == _lib.COREG_EINVAL
    assert fn(h._h, v.ctypes.data, -32, ny * nx, ny, nx, idx.ctypes.data, 3, C.byref(p), None, None, None) == _lib.COREG_EINVAL
    assert fn(h._h, v.ctypes.data, -32, ny * nx, ny, nx, idx.ctypes.data, 3, None, out.ctypes.data, None, None) == _lib.COREG_EINVAL
    assert (out == -7.0).all()
    # the events and the counts may be left out
    assert fn(h._h, v.ctypes.data, -32, ny * nx, ny, nx, idx.ctypes.data, 3, C.byref(p), out.ctypes.data, None, None) == 0
    assert np.array_equal(out, PO.despike_sum_planes(np.asarray(v, dtype=np.float32), **good)[0], equal_nan=True)


# ---- 5. what it is for -------------------------------------------------------------------------------------------------
def test_the_hits_of_the_precondition_are_marked_on_the_device(gpu_handle):
    planes, mask, *_ = hit_cube()
    want = PO.despike_sum_planes(planes, **HIT_RULE)
    s, events, counts = gpu_handle.despike_sum_planes(PO.be(planes), np.arange(len(planes)), HIT_RULE)
    assert np.array_equal(s, want[0], equal_nan=True) and np.array_equal(events, want[1]) and counts == want[2]
    marked = int(((events > 0) & mask).sum())
    print(f"[despike planes] {marked} of {N_HITS} hit pixels marked on the device")
    assert marked >= 50


# ---- 6. the classes ----------------------------------------------------------------------------------------------------
INTERVAL = [976.74, 977.22]  # planes 1 .. 5 of the 8
LAG1, LAG2 = np.array([-27.0, -23.0, -19.0]), np.array([32.0, 36.0, 40.0])
CLASS_RULE = dict(radius=2, n_iter=2, nsigma=5.0, floor=0.0, min_neighbours=5, sign="positive", replace="median")


@pytest.fixture(scope="module")
def spice():
    """The precondition's cube as a SPICE L2 window, the five planes the interval selects, the slit rows, and the oracle's
    sum of those planes over those rows placed in an image that is NaN elsewhere -- computed once."""
    from euispice_coreg_amd.utils import spice_header
    planes, mask, h4, large, hl = hit_cube()
    wave = spice_header.wavelengths_angstrom(fits_header(h4))
    sel = np.flatnonzero((wave >= INTERVAL[0]) & (wave <= INTERVAL[1]))
    assert list(sel) == [1, 2, 3, 4, 5]
    ymin, ymax, _ = slice(*spice_header.vertical_edges_limits(fits_header(h4))).indices(planes.shape[1])
    assert 0 < ymin < ymax <= planes.shape[1]  # (rows below ymin are cut: they must never be neighbours)
    s, e, counts = PO.despike_sum_planes(planes[sel][:, ymin:ymax], **CLASS_RULE)
    image = np.full(planes.shape[1:], np.nan)
    events = np.zeros(planes.shape[1:], dtype=np.int32)
    image[ymin:ymax], events[ymin:ymax] = s, e
    assert counts[0] >= 20
    plain = np.nansum(planes[sel].astype(np.float64), axis=0)
    plain[:ymin] = np.nan
    plain[ymax:] = np.nan
    return dict(cube=planes[None], h4=h4, large=large, hl=hl, sel=sel, rows=(ymin, ymax), image=image, events=events,
                counts=counts, plain=plain, mask=mask)


def fits_header(h):
    from euispice_coreg_amd.utils import fits_io
    return fits_io.Header(h)


def _spice_kw():
    return dict(lag_crval1=LAG1, lag_crval2=LAG2, parallelism=True, level=2, wavelength_interval_to_sum=INTERVAL)


def test_alignment_spice_sums_the_despiked_planes(spice):
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    m = spice
    A = AlignmentSpice((m["large"], m["hl"]), (m["cube"], m["h4"]), despike_planes=CLASS_RULE, **_spice_kw())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = A.align_using_helioprojective(method="correlation", return_type="corr")
    assert np.array_equal(A.data_small, m["image"], equal_nan=True)
    assert A.last_despiked_planes == m["counts"] and np.array_equal(A.despiked_plane_events, m["events"])
    assert A.despiked_plane_events.dtype == np.int32 and not np.array_equal(m["image"], m["plain"], equal_nan=True)
    lags = (LAG1, LAG2, [0.0], [0.0], [0.0])
    want = H.oracle_helio(m["image"], A.hdr_small, m["large"], m["hl"], lags, parallelism=True, unit_lag="arcsec")
    H.assert_corr_close(got, want, 1e-7, "AlignmentSpice, despike_planes, helioprojective")
    assert np.isfinite(want).all() and A.last_despiked == {"small": [], "large": []}
    B = AlignmentSpice((m["large"], m["hl"]), (m["cube"], m["h4"]), despike_planes=CLASS_RULE, **_spice_kw())
    kw = dict(lonlims=(242.5, 245.5), latlims=(5.0, 7.5), shape=(30, 40))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gotc = B.align_using_carrington(**kw, return_type="corr")
    assert np.array_equal(B.data_small, m["image"], equal_nan=True) and B.last_despiked_planes == m["counts"]
    wantc = H.oracle_carrington(m["image"], B.hdr_small, m["large"], m["hl"], (LAG1, LAG2, None, None, None), kw["shape"],
                                kw["lonlims"], kw["latlims"])
    H.assert_corr_close(gotc, wantc, 1e-10, "AlignmentSpice, despike_planes, carrington")
    assert np.isfinite(wantc).any()


def test_without_the_keyword_the_host_sum_is_what_it_was(spice):
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    m = spice
    for cube in (m["cube"], PO.be(m["cube"])):  # (NumPy's additions; the library's host routine on big-endian planes)
        A = AlignmentSpice((m["large"], m["hl"]), (cube, m["h4"]), **_spice_kw())
        A._extract_imager_data_header()
        A._extract_spice_data_header(level=2)
        assert A.data_small.tobytes() == m["plain"].tobytes()
        assert A.despike_planes is None and A.last_despiked_planes is None and A.despiked_plane_events is None


def test_planes_first_then_the_summed_image(spice):
    """despike_planes with despike_small: the planes, the sum, then the summed image; counts in both attributes."""
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    m = spice
    A = AlignmentSpice((m["large"], m["hl"]), (m["cube"], m["h4"]), despike_planes=CLASS_RULE, despike_small=True,
                       **_spice_kw())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = A.align_using_helioprojective(method="correlation", return_type="corr")
    assert np.array_equal(A.data_small, m["image"], equal_nan=True) and A.last_despiked_planes == m["counts"]
    small_d, counts_s = DO.despike(m["image"], **DO.DEFAULTS)
    assert sorted(A.last_despiked) == ["large", "small"] and A.last_despiked == {"small": counts_s, "large": []}
    want = H.oracle_helio(small_d, A.hdr_small, m["large"], m["hl"], (LAG1, LAG2, [0.0], [0.0], [0.0]), parallelism=True,
                          unit_lag="arcsec")
    H.assert_corr_close(got, want, 1e-7, "AlignmentSpice, despike_planes and despike_small")


def test_level_3_with_the_keyword_is_refused(spice):
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    m = spice
    A = AlignmentSpice((m["large"], m["hl"]), (m["cube"], m["h4"]), lag_crval1=LAG1, lag_crval2=LAG2, level=3,
                       despike_planes=True)
    with pytest.raises(ValueError) as e:
        A.align_using_helioprojective(coefficient_l3=0)
    assert "despike_planes" in str(e.value)


def _write_spice(m, tmp_path):
    from euispice_coreg_amd.utils import fits_io
    p_spice = str(tmp_path / "solo_L2_spice-n-ras_20220317T094045_V01.fits")
    fits_io.write_images(p_spice, [(m["cube"], m["h4"])])
    return p_spice


def test_alignment_spice_pixel_sums_the_despiked_planes(spice, tmp_path):
    from euispice_coreg_amd.pxlshift import AlignmentSpicePixel
    from euispice_coreg_amd.utils import fits_io
    m = spice
    p_spice = _write_spice(m, tmp_path)
    p_fsi = str(tmp_path / "solo_L2_eui-fsi174-image_ref.fits")
    fits_io.write_images(p_fsi, [(None, {}), (np.asarray(m["large"], dtype=np.float32), m["hl"])])
    prm = dict(CLASS_RULE, n_iter=1)
    A = AlignmentSpicePixel(p_fsi, 1, p_spice, 0, despike_planes=prm)
    B = AlignmentSpicePixel(p_fsi, 1, p_spice, 0)
    ylim, ylen = A.row_offset, m["cube"].shape[2]
    assert ylim > 0 and B.row_offset == ylim and B.last_despiked_planes is None and B.despiked_plane_events is None
    want = PO.despike_sum_planes(m["cube"][0][:, ylim:ylen - ylim], **prm)
    assert np.array_equal(A.data_small, want[0], equal_nan=True) and A.data_small.shape == B.data_small.shape
    assert np.array_equal(A.despiked_plane_events, want[1]) and A.last_despiked_planes == want[2] and want[2][0] >= 20
    assert B.data_small.tobytes() == np.nansum(m["cube"][0][:, ylim:ylen - ylim].astype(np.float64), axis=0).tobytes()


def test_iterative_context_sums_the_despiked_planes(spice, tmp_path):
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.hdrshift import AlignementSpiceIterativeContextRaster
    from euispice_coreg_amd.utils import fits_io
    m = spice
    p_spice = _write_spice(m, tmp_path)
    paths = []
    for j, (img, hdr) in enumerate(synthetic.make_imager_sequence(m["large"], m["hl"], n_frames=3)):
        p = str(tmp_path / f"solo_L2_eui-fsi174-image_{j:02d}.fits")
        fits_io.write_images(p, [(None, {}), (img, hdr)])
        paths.append(p)
    kw = dict(large_fov_list_paths=paths, small_fov_to_correct=p_spice, threshold_time=1e6, lag_crval1=np.array([-23.0]),
              lag_crval2=np.array([36.0]), lag_cdelt1=None, lag_cdelt2=None, lag_crota=None, small_fov_window=0)
    A = AlignementSpiceIterativeContextRaster(despike_planes=dict(CLASS_RULE, n_iter=1), **kw)
    B = AlignementSpiceIterativeContextRaster(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = np.asarray(A.align_using_helioprojective(method="correlation").corr)
        plain = np.asarray(B.align_using_helioprojective(method="correlation").corr)
    ymin, ymax = m["rows"]
    want = PO.despike_sum_planes(m["cube"][0][:, ymin:ymax], **dict(CLASS_RULE, n_iter=1))
    image = np.full(m["image"].shape, np.nan)
    image[ymin:ymax] = want[0]
    assert np.array_equal(A.data_small, image, equal_nan=True) and A.last_despiked_planes == want[2]
    assert np.array_equal(A.despiked_plane_events[ymin:ymax], want[1]) and not A.despiked_plane_events[:ymin].any()
    whole = np.nansum(m["cube"][0].astype(np.float64), axis=0)
    whole[:ymin] = np.nan
    whole[ymax:] = np.nan
    assert B.data_small.tobytes() == whole.tobytes() and B.last_despiked_planes is None
    assert np.isfinite(got).all() and np.isfinite(plain).all() and not np.array_equal(got, plain)
    l3 = AlignementSpiceIterativeContextRaster(despike_planes=True, **dict(kw, small_fov_to_correct="solo_L3_spice-n-ras.fits"))
    with pytest.raises(ValueError):
        l3.align_using_helioprojective()
