"""
GPU tests of the pixel-lag alignment (pxlshift): every case of tests/golden/pxlshift_golden.* through the public
classes, against the reference's own output.

Tolerance, derived: a float64 summation in another order moves the quotient by at most n 2^-53 (Cauchy-Schwarz; n <=
9100 pixels here: 1e-12), and when the two numerators straddle a float32 rounding boundary the entry moves by one
float32 ulp, 2^-23 |corr|.  So every entry is within 2^-23 |corr_ref| + 1e-12, and at most 1 entry in 100 of a cube's
unrotated planes may need more than 1e-12 (rotated planes: 1e-10, a libm difference of ~1e-13 px in a coordinate
reaches the sample through the image gradient) -- the cap keeps the ulp allowance from hiding a wrong numerator.
"""
import numpy as np
import pytest

from . import pxlshift_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every sweep case once: (object, cube, sub-resolved box, rotated plane or None)."""
    _, meta = Cs.golden()
    out = {}
    for name in Cs.SWEEP_CASES:
        A, kw = Cs.make(name, tmp_path_factory.mktemp("pxl_" + name))
        corr = A.find_best_parameters(**kw)
        k = meta["cases"][name].get("rotated_index")
        out[name] = (A, kw, corr, A._large_box(), None if k is None else A._rotated(k))
    return out


@pytest.mark.parametrize("name", Cs.SWEEP_CASES)
def test_cube_against_reference(name, runs):
    arr, meta = Cs.golden()
    c, want = meta["cases"][name], arr[f"{name}/corr"]
    got = runs[name][2]
    assert got.dtype == np.float64 and got.shape == want.shape == tuple(c["shape"]) and got.flags.c_contiguous
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanargmax(got) == np.nanargmax(want)
    d = np.abs(got - want)
    rot = np.array(c["lag_drot"]) != 0
    print(name, "max |diff|", d.max(), "unrotated entries > 1e-12:", int((d[:, :, ~rot] > 1e-12).sum()), "of",
          d[:, :, ~rot].size, "rotated entries > 1e-10:", int((d[:, :, rot] > 1e-10).sum()), "of", d[:, :, rot].size)
    assert np.all(d <= 2.0 ** -23 * np.abs(want) + 1e-12)
    assert (d[:, :, ~rot] > 1e-12).sum() <= d[:, :, ~rot].size / 100
    assert (d[:, :, rot] > 1e-10).sum() <= d[:, :, rot].size / 100


@pytest.mark.parametrize("name", Cs.SWEEP_CASES)
def test_sub_resolved_box_to_the_bit(name, runs):
    arr, _ = Cs.golden()
    got, want = runs[name][3], arr[f"{name}/large_box"]
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("name", ["a", "b"])
def test_rotated_plane(name, runs):
    arr, _ = Cs.golden()
    got, want = runs[name][4], arr[f"{name}/data_small_rotated"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = np.nanmax(np.abs(got - want))
    print(name, "rotated plane: max |diff|", err)
    assert err <= 1e-9 * np.nanmax(np.abs(runs[name][0].data_small))


def test_batching_invariance(runs):
    """Case b in one call and as two calls cut along dx at an odd index: the same bits."""
    A, kw, whole = runs["b"][:3]
    cut = 7
    parts = [A.find_best_parameters(**dict(kw, lag_dx=kw["lag_dx"][:cut])),
             A.find_best_parameters(**dict(kw, lag_dx=kw["lag_dx"][cut:]))]
    assert np.array_equal(np.concatenate(parts, axis=0), whole, equal_nan=True)


def test_second_call_on_one_object(runs):
    for name in ("a", "d_crota"):  # (d: the displacement of the large image is not applied twice)
        A, kw, first = runs[name][:3]
        assert np.array_equal(A.find_best_parameters(**kw), first, equal_nan=True)


def test_flat_image_and_out_of_bounds(tmp_path):
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    arr, meta = Cs.golden()
    c = meta["cases"]["f"]
    _, hs, large, hl = Cs.inputs("a")
    pl, ps = Cs.write_pair(tmp_path, "f", np.full(c["small_shape"], c["small_value"]), hs, large, hl)
    A = AlignmentPixels(pl, 0, ps, 0)
    got = A.find_best_parameters(np.array(c["lag_dx"]), np.array(c["lag_dy"]), np.array(c["lag_drot"]))
    assert got.shape == tuple(c["shape"]) and np.isnan(got).all() and np.isnan(arr["f/corr"]).all()
    o = c["out_of_bounds"]
    with pytest.raises(ValueError, match=o["message"]):
        A.find_best_parameters(np.array(o["lag_dx"]), np.array(o["lag_dy"]), np.array([0.0]))
