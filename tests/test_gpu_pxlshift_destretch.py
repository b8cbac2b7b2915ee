"""
GPU tests of the destretch of a local shift field (`LocalShiftField.destretch`, coreg_pixels_destretch,
k_pixels_destretch of csrc/kernels_pixels.hpp) against tests/pxlshift_destretch_oracle.py.  Every comparison is bit for
bit -- the displacement, and the planes in float64 and in float32, NaN pattern included: every step of the rule is one
IEEE operation in a fixed order.

The shapes are the smallest that walk each path (a thread owns an output pixel, a workgroup 256 of them, and
blockIdx.y deals chunks of kPixDsPlanes = 8 planes, the last one short): a 5 x 7 stack of one plane, a 37 x 70 image
(width no multiple of 64, eleven workgroups) with 1 and with 19 planes, a one-row image, one node on either axis, ragged
last tiles, offsets on a cube taller than the field's image, integer nodes under "nearest" that put coordinates exactly on
n - 1 and one pixel beyond, NaN pixels next to weight-0 taps, both interpolations.
"""
import ctypes as C

import numpy as np
import pytest

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import LocalShiftField

from . import pxlshift_destretch_cases as DC
from . import pxlshift_destretch_oracle as D
from . import pxlshift_tiles_cases as TC

pytestmark = pytest.mark.gpu

CHUNK = 8  # kPixDsPlanes
INTERPOLATIONS = ("bilinear", "nearest")


@pytest.fixture(scope="module")
def hnd():
    with _lib.CoregHandle(0) as h:
        yield h


def _same_bits(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits))


def _centres(n, t):
    """The centres of tiles of t pixels on an axis of n (the last one ragged)."""
    return np.array([(a + min(n, a + t) - 1) / 2 for a in range(0, n, t)], dtype=np.float64)


def _cube(rng, n_planes, ny, nx, dtype, n_nan):
    cube = rng.uniform(1.0, 9.0, (n_planes, ny, nx)).astype(dtype)
    cube[rng.integers(0, n_planes, n_nan), rng.integers(0, ny, n_nan), rng.integers(0, nx, n_nan)] = np.nan
    return cube


def _field(rng, field_shape, tile):
    """Nodes at the centres of the tiles of `tile` on an image of `field_shape`: random shifts of up to 3 px, the first
    two columns of nodes whole numbers (taps of weight 0 between them)."""
    ys, xs = _centres(field_shape[0], tile[0]), _centres(field_shape[1], tile[1])
    u, v = rng.uniform(-3, 3, (len(ys), len(xs))), rng.uniform(-3, 3, (len(ys), len(xs)))
    u[:, :2], v[:, :2] = 1.0, -2.0
    return ys, xs, u, v


def _check(hnd, cube, ys, xs, u, v, tile, row_offset=0.0, col_offset=0.0, label=""):
    for interp in INTERPOLATIONS:
        want, wd = D.destretch(cube, ys, xs, u, v, tile, interp, row_offset, col_offset)
        got, gd = hnd.pixels_destretch(cube, ys, xs, u, v, tile, INTERPOLATIONS.index(interp), row_offset, col_offset,
                                       return_displacement=True)
        print(label, interp, cube.dtype, cube.shape, "nodes", u.shape, "NaN", int(np.isnan(want).sum()), "of", want.size)
        assert _same_bits(gd, wd), (label, interp, "displacement")
        assert _same_bits(got, want), (label, interp, "planes")
        assert 0 < np.isnan(want).sum() < want.size
        again = hnd.pixels_destretch(cube, ys, xs, u, v, tile, INTERPOLATIONS.index(interp), row_offset, col_offset)
        assert _same_bits(again, want)  # (without the displacement)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_small_stack_of_one_plane(hnd, dtype):
    """5 x 7, one plane, tiles of (3, 4): 2 x 2 nodes, ragged on both axes."""
    rng = np.random.default_rng(40)
    cube = _cube(rng, 1, 5, 7, dtype, 2)
    ys, xs, u, v = _field(rng, (5, 7), (3, 4))
    assert ys.tolist() == [1.0, 3.5] and xs.tolist() == [1.5, 5.0]
    _check(hnd, cube, ys, xs, u * 0.4, v * 0.4, (3, 4), label="5 x 7")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_planes", [1, 2 * CHUNK + 3])
def test_an_image_of_several_workgroups(hnd, dtype, n_planes):
    """37 x 70 (2590 pixels: eleven workgroups, the last one short; a width that is no multiple of 64), tiles of (10, 16):
    4 x 5 nodes with ragged last tiles; one plane, and 19 planes (two whole chunks and a short one)."""
    rng = np.random.default_rng(41)
    cube = _cube(rng, n_planes, 37, 70, dtype, 12 * n_planes)
    ys, xs, u, v = _field(rng, (37, 70), (10, 16))
    assert u.shape == (4, 5) and ys[-1] == 33.0 and xs[-1] == 66.5
    _check(hnd, cube, ys, xs, u, v, (10, 16), label="37 x 70")


def test_a_one_row_image_and_one_node_on_either_axis(hnd):
    rng = np.random.default_rng(42)
    row = _cube(rng, 3, 1, 70, np.float32, 4)
    ys, xs, u, v = _field(rng, (1, 70), (1, 16))
    assert u.shape == (1, 5)
    _check(hnd, row, ys, xs, u, v * 0.0, (1, 16), label="1 x 70")  # (any v != 0 leaves a one-row image)
    cube = _cube(rng, 2, 37, 70, np.float64, 20)
    ys, xs, u, v = _field(rng, (37, 70), (37, 16))  # one node along y
    assert u.shape == (1, 5)
    _check(hnd, cube, ys, xs, u, v, (37, 16), label="1 x 5 nodes")
    ys, xs, u, v = _field(rng, (37, 70), (10, 70))  # one node along x
    assert u.shape == (4, 1)
    _check(hnd, cube, ys, xs, rng.uniform(-3, 3, (4, 1)), v, (10, 70), label="4 x 1 nodes")
    ys, xs, u, v = _field(rng, (37, 70), (37, 70))  # one node
    assert u.shape == (1, 1)
    _check(hnd, cube, ys, xs, np.array([[0.75]]), np.array([[-1.5]]), (37, 70), label="1 x 1 node")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_offsets_on_a_cube_taller_than_the_field(hnd, dtype):
    """The field of a 37 x 64 image on planes of 45 x 70 whose pixel (4, 3) is the image's first: rows and columns outside
    the field take the values of its outer nodes (bilinear) or outer tiles (nearest)."""
    rng = np.random.default_rng(43)
    cube = _cube(rng, CHUNK + 1, 45, 70, dtype, 60)
    ys, xs, u, v = _field(rng, (37, 64), (10, 16))
    _check(hnd, cube, ys, xs, u, v, (10, 16), row_offset=4, col_offset=3, label="offsets")
    _check(hnd, cube, ys, xs, u, v, (10, 16), row_offset=-2.5, col_offset=0.25, label="fractional offsets")


def test_coordinates_on_the_last_pixel_and_beyond_and_weight_zero_taps(hnd):
    """One tile, "nearest" (and bilinear, one node: the same constant), whole-number nodes: D(Y, X) = S(Y + 2, X + 1).  Row
    3 of the 5 x 6 result samples row n - 1 exactly (the mirrored tap), row 4 one pixel beyond (NaN), likewise the columns;
    a NaN at (3, 5) reaches six samples through taps of weight 0."""
    img = (np.arange(30, dtype=np.float64).reshape(1, 5, 6) + 1.0)
    ys, xs, u, v = np.array([2.0]), np.array([2.5]), np.array([[-1.0]]), np.array([[-2.0]])
    for dtype in (np.float64, np.float32):
        a = img.astype(dtype)
        got = hnd.pixels_destretch(a, ys, xs, u, v, (5, 6), 1)
        assert np.array_equal(got[0, :3, :5], a[0, 2:, 1:]) and np.isnan(got[0, 3:]).all() and np.isnan(got[0, :, 5]).all()
        a[0, 3, 5] = np.nan
        _check(hnd, a, ys, xs, u, v, (5, 6), label="edges")
        got = hnd.pixels_destretch(a, ys, xs, u, v, (5, 6), 1)
        assert np.isnan(got[0, :3, :5]).sum() == 6 and np.isnan(got[0, 2, 3]) and np.isfinite(got[0, 2, 2])


# ---------------------------------------------------------------------------------------------------- public interface
def test_field_destretch_of_a_stack(hnd):
    """`LocalShiftField.destretch` on a stack [2, 3, 45, 70] of float32 (big-endian, as a FITS data unit) with offsets,
    against the oracle on the field's own nodes."""
    rng = np.random.default_rng(44)
    lag = np.arange(-3, 4)
    corr = rng.uniform(0.1, 0.9, (4, 4, 7, 7, 1))
    F = LocalShiftField(corr, np.full(corr.shape, 160.0), lag, lag, [0.0], (10, 16), (37, 64), sub_lag=False)
    stack = _cube(rng, 6, 45, 70, np.float32, 40).reshape(2, 3, 45, 70).astype(">f4")
    for interp in INTERPOLATIONS:
        got, disp = F.destretch(stack, interpolation=interp, row_offset=4, col_offset=3, return_displacement=True)
        want = D.field_destretch(F, stack, interpolation=interp, row_offset=4, col_offset=3)
        assert got.shape == stack.shape and _same_bits(got, want) and disp.shape == (2, 45, 70)


def test_closed_loop_two_drift_scene_end_to_end():
    """find_local_shifts, destretch, find_local_shifts: exactly the reference in every tile."""
    A, kw, ts, want = TC.two_drift_object()
    F = A.find_local_shifts(**kw, tile_shape=ts, sub_lag=False)
    want = np.array(want)
    assert np.array_equal(F.shift_dx, want[..., 0]) and np.array_equal(F.shift_dy, want[..., 1])
    for ref in ((0, 0), (2, -1)):
        d = F.destretch(A.data_small, reference=ref, interpolation="nearest")
        assert _same_bits(d, D.field_destretch(F, A.data_small, reference=ref, interpolation="nearest"))
        G = DC.pair(A.data_large, d).find_local_shifts(**kw, tile_shape=ts, sub_lag=False)
        print(ref, "dx", G.shift_dx.tolist(), "dy", G.shift_dy.tolist(), "lowest best score", G.best_score.min())
        assert G.valid.all() and (G.shift_dx == ref[0]).all() and (G.shift_dy == ref[1]).all()


def test_the_sweep_state_is_untouched():
    A, kw, ts, _ = TC.two_drift_object()
    F = A.find_local_shifts(**kw, tile_shape=ts, sub_lag=False)
    cube = A.find_best_parameters(**kw)
    counts = A.last_counts.copy()
    with _lib.CoregHandle(0) as h:
        plan = A.host_plan(**kw)
        h.pixels_set_large(A.data_large)
        h.pixels_set_small(A.data_small)
        first = h.pixels_sweep(plan, plan["method_code"])
        assert np.array_equal(first, cube, equal_nan=True)
        box, timing = h.pixels_get_large_box((48, 56)), h.pixels_last_timing()
        u, v = F.node_shifts()
        h.pixels_destretch(A.data_small[None], F.tile_centres[:, 0, 1], F.tile_centres[0, :, 0], u, v, ts)
        assert h.pixels_destretch_last_ms() >= 0.0
        # the resident images, the counts and the times of the sweep are those of before
        assert np.array_equal(h.pixels_last_counts(first.shape), counts)
        assert np.array_equal(h.pixels_get_large_box((48, 56)), box, equal_nan=True) and h.pixels_last_timing() == timing
        assert np.array_equal(h.pixels_get_rotated(0, A.data_small.shape), A.data_small, equal_nan=True)
        assert np.array_equal(h.pixels_sweep(plan, plan["method_code"]), cube, equal_nan=True)  # (no image set again)
    F.destretch(A.data_small)
    assert np.array_equal(A.find_best_parameters(**kw), cube, equal_nan=True) and np.array_equal(A.last_counts, counts)


def _code(fn, *args, **kw):
    with pytest.raises(_lib.CoregError) as e:
        fn(*args, **kw)
    assert str(e.value).split(": ", 1)[1]  # (every refusal leaves a message)
    return e.value.code


def test_refusals_of_the_c_call():
    cube = np.ones((2, 5, 7))
    ys, xs, u, v = np.array([1.0, 3.5]), np.array([1.5, 5.0]), np.zeros((2, 2)), np.zeros((2, 2))
    nan_u = u.copy()
    nan_u[1, 0] = np.nan
    with _lib.CoregHandle(0) as h:
        assert _code(h.pixels_destretch_last_ms) == _lib.COREG_ESTATE  # a fresh handle
        for bad in ((cube, ys, xs[::-1], u, v, (3, 4)), (cube, ys, np.array([1.5, 1.5]), u, v, (3, 4)),
                    (cube, np.array([1.0, np.nan]), xs, u, v, (3, 4)), (cube, ys[::-1], xs, u, v, (3, 4)),
                    (cube, ys, xs, nan_u, v, (3, 4)), (cube, ys, xs, u, np.full((2, 2), np.inf), (3, 4)),
                    (cube, ys, xs, u, v, (3, 4), 2), (cube, ys, xs, u, v, (3, 4), -1), (cube, ys, xs, u, v, (0, 4)),
                    (cube, ys, xs, u, v, (3, 4), 0, np.nan), (cube, ys, xs, u, v, (3, 4), 0, 0.0, np.inf)):
            assert _code(h.pixels_destretch, *bad) == _lib.COREG_EINVAL
        assert _code(h.pixels_destretch_last_ms) == _lib.COREG_ESTATE  # (a refused call has not run)
        # more than 2^31 - 1 elements: refused from the shape alone, before the cube is read
        f = _lib.PixelsField(2, 2, 3, 4, 0, _lib._dptr(ys), _lib._dptr(xs), _lib._dptr(u), _lib._dptr(v), 0.0, 0.0)
        out = np.empty_like(cube)
        lib = _lib.load_library()
        for shape in ((70000, 5, 7000), (2, 50000, 50000), (2 ** 31 - 1, 1, 2)):
            assert lib.coreg_pixels_destretch(h._h, cube.ctypes.data, _lib.COREG_F64, *shape, C.byref(f), out.ctypes.data,
                                              None) == _lib.COREG_EINVAL
        assert lib.coreg_pixels_destretch(h._h, cube.ctypes.data, 7, 2, 5, 7, C.byref(f), out.ctypes.data, None) == _lib.COREG_EINVAL
        assert lib.coreg_pixels_destretch(h._h, None, _lib.COREG_F64, 2, 5, 7, C.byref(f), out.ctypes.data, None) == _lib.COREG_EINVAL
        assert lib.coreg_pixels_destretch(None, cube.ctypes.data, _lib.COREG_F64, 2, 5, 7, C.byref(f), out.ctypes.data,
                                          None) == _lib.COREG_EINVAL
        assert _code(h.pixels_last_timing) == _lib.COREG_ESTATE  # no sweep has run: the destretch leaves no sweep times
        got = h.pixels_destretch(cube, ys, xs, u, v, (3, 4))  # zero nodes: the cube itself
        assert np.array_equal(got, cube) and h.pixels_destretch_last_ms() >= 0.0
