"""
CPU tests of the pixel-lag alignment (pxlshift): the numpy restatement tests/pxlshift_oracle.py against the reference's
own output (tests/golden/pxlshift_golden.*), and the host part of the public classes -- plan, preparation of the SPICE
image, error cases, align_pixels_shift -- against the same.  No GPU.

Bounds (from the issue, not from the code under test): unrotated planes are reproduced exactly; on rotated planes a
libm difference in a coordinate may move the float32-rounded numerator by one float32 ulp: 2^-23 |corr| + 1e-12, and at
most 1 entry in 100 per cube may need more than 1e-10.
"""
import numpy as np
import pytest

from euispice_coreg_amd.pxlshift import AlignmentPixels, AlignmentSpicePixel, align_pixels_shift
from euispice_coreg_amd.utils import fits_io

from . import pxlshift_cases as Cs
from . import pxlshift_oracle as O


def _case_images(name):
    arr, meta = Cs.golden()
    c = meta["cases"][name]
    if name == "e":
        return arr["e/data_small"], arr["e/large"].astype(np.float64), c
    small, _, large, _ = Cs.inputs(name)
    if name.startswith("d_"):
        large = O.shift_large(large, c["printed_dx"], c["printed_dy"])
    return small, large, c


@pytest.fixture(scope="module")
def oracle_cubes():
    """The restatement's sub-resolved image and cube of every sweep case, computed once."""
    out = {}
    for name in Cs.SWEEP_CASES:
        small, large, c = _case_images(name)
        sub = O.sub_resolution(large, c["ratio_res_1"], c["ratio_res_2"])
        out[name] = (sub, O.sweep(sub, small, c["lag_dx"], c["lag_dy"], c["lag_drot"], c["unit_rot"]))
    return out


@pytest.mark.parametrize("name", Cs.SWEEP_CASES)
def test_oracle_reproduces_golden_cube(name, oracle_cubes):
    arr, meta = Cs.golden()
    c, want = meta["cases"][name], arr[f"{name}/corr"]
    sub, got = oracle_cubes[name]
    assert list(sub.shape) == c["sub_shape"]
    assert got.shape == want.shape == tuple(c["shape"]) and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanargmax(got) == np.nanargmax(want)
    for k, drot in enumerate(c["lag_drot"]):
        d = np.abs(got[:, :, k] - want[:, :, k])
        print(name, "drot", drot, "max |diff|", d.max(), "entries > 1e-10:", int((d > 1e-10).sum()), "of", d.size)
        if drot == 0:
            assert d.max() == 0.0
        else:
            assert np.all(d <= 2.0 ** -23 * np.abs(want[:, :, k]) + 1e-12)
    d = np.abs(got - want)
    assert (d > 1e-10).sum() <= d.size / 100


@pytest.mark.parametrize("name", Cs.SWEEP_CASES)
def test_oracle_reproduces_sub_resolved_box(name, oracle_cubes):
    arr, meta = Cs.golden()
    c = meta["cases"][name]
    sub, _ = oracle_cubes[name]
    want = arr[f"{name}/large_box"]
    l, dx, dy = c["slc_small_ref"], c["lag_dx"], c["lag_dy"]
    h, w = want.shape[0] - (max(dy) - min(dy)), want.shape[1] - (max(dx) - min(dx))
    got = sub[l[0] + min(dy):l[0] + h + max(dy), l[1] + min(dx):l[1] + w + max(dx)]
    assert np.array_equal(got, want, equal_nan=True)
    assert O.slice_origin(sub.shape, (h, w)) == l


@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_reproduces_rotated_plane(name):
    arr, meta = Cs.golden()
    c = meta["cases"][name]
    small = Cs.inputs(name)[0]
    want = arr[f"{name}/data_small_rotated"]
    got = O.rotate(small, c["lag_drot"][c["rotated_index"]], c["unit_rot"])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-9 * np.nanmax(np.abs(small))


@pytest.mark.parametrize("name", ["d_crota", "d_nocrota"])
def test_oracle_reproduces_shifted_image(name):
    arr, meta = Cs.golden()
    c = meta["cases"][name]
    large = Cs.inputs(name)[2]
    assert np.array_equal(O.shift_large(large, c["printed_dx"], c["printed_dy"]), arr[f"{name}/shifted"], equal_nan=True)


def test_flat_image_restated():
    arr, meta = Cs.golden()
    c = meta["cases"]["f"]
    large = arr["a/large"].astype(np.float64)
    sub = O.sub_resolution(large, 0.9, 0.8)
    got = O.sweep(sub, np.full(c["small_shape"], c["small_value"]), c["lag_dx"], c["lag_dy"], c["lag_drot"])
    assert np.isnan(arr["f/corr"]).all() and np.isnan(got).all() and got.shape == tuple(c["shape"])


# ------------------------------------------------------------------------------------------------------ host plan
@pytest.mark.parametrize("name", Cs.SWEEP_CASES)
def test_host_plan_equals_golden(name, tmp_path):
    _, meta = Cs.golden()
    c = meta["cases"][name]
    A, kw = Cs.make(name, tmp_path)
    p = A.host_plan(**kw)
    assert float(p["ratio_res_1"]).hex() == c["ratio_res_1_hex"]
    assert float(p["ratio_res_2"]).hex() == c["ratio_res_2_hex"]
    assert list(p["sub_shape"]) == c["sub_shape"]
    assert list(p["slc_small_ref"]) == c["slc_small_ref"]
    h, w = A.data_small.shape
    assert (p["xc"], p["yc"]) == (round(w / 2), round(h / 2))
    if c["unit_rot"] == "degree":
        assert np.array_equal(p["lag_drot_rad"], np.radians(np.array(c["lag_drot"])))
    else:
        assert np.array_equal(p["lag_drot_rad"], np.array(c["lag_drot"]))
    if name.startswith("d_"):
        dx, dy = p["shift_large"]
        assert abs(dx - c["printed_dx"]) <= 1e-12 * abs(c["printed_dx"])
        assert abs(dy - c["printed_dy"]) <= 1e-12 * abs(c["printed_dy"])
        assert (dy == 0.0) == (name == "d_nocrota")
    else:
        assert p["shift_large"] is None


def test_centre_rounds_half_to_even(tmp_path):
    small, hs, large, hl = Cs.inputs("a")
    pl, ps = Cs.write_pair(tmp_path, "r", small[:, :-4], hs, large, hl)
    A = AlignmentPixels(pl, 0, ps, 0)
    p = A.host_plan([0], [0], [0.0])  # 25 x 17: 17 / 2 = 8.5 -> 8, 25 / 2 = 12.5 -> 12
    assert (p["xc"], p["yc"]) == (8, 12)


def test_edges_and_one_lag_beyond(tmp_path):
    _, meta = Cs.golden()
    c = meta["cases"]["c"]
    A, kw = Cs.make("c", tmp_path)
    p = A.host_plan(**kw)
    l, sub = p["slc_small_ref"], p["sub_shape"]
    h, w = A.data_small.shape
    # the ranges reach the edges exactly
    assert l[1] + min(c["lag_dx"]) == 0 and l[1] + w + max(c["lag_dx"]) == sub[1]
    assert l[0] + min(c["lag_dy"]) == 0 and l[0] + h + max(c["lag_dy"]) == sub[0]
    assert len(c["beyond"]) == 4
    for b in c["beyond"]:
        with pytest.raises(ValueError, match="too large shift : outside FSI"):
            A.host_plan(b["lag_dx"], b["lag_dy"], [0.0])
        with pytest.raises(ValueError, match="too large shift : outside FSI"):  # raised before any GPU work
            A.find_best_parameters(np.array(b["lag_dx"]), np.array(b["lag_dy"]), np.array([0.0]))


def test_error_cases(tmp_path):
    _, meta = Cs.golden()
    f = meta["cases"]["f"]["out_of_bounds"]
    A, _ = Cs.make("a", tmp_path)
    with pytest.raises(ValueError, match=f["message"]):
        A.host_plan(f["lag_dx"], f["lag_dy"], [0.0])
    with pytest.raises(TypeError):
        A.host_plan(np.array([0.5, 1.0]), [0], [0.0])
    with pytest.raises(TypeError):
        A.host_plan([0], np.array([0.25]), [0.0])
    with pytest.raises(ValueError, match="unit_rot"):
        A.host_plan([0], [0], [1.0], unit_rot="grad")
    with pytest.raises(KeyError):  # shift_solar_rotation_dx_large without the keywords it reads
        A.hdr_large.pop("WAVELNTH")
        A.host_plan([0], [0], [0.0], shift_solar_rotation_dx_large=True)
    assert A.host_plan(np.array([1.0, 2.0]), [0], [0.0])["lag_dx"].tolist() == [1, 2]  # integer-valued floats


def test_level3_is_not_implemented(tmp_path):
    p_fsi, _ = Cs.write_spice(tmp_path)
    with pytest.raises(NotImplementedError, match="level-3"):
        AlignmentSpicePixel(p_fsi, 1, str(tmp_path / "solo_L3_spice-n-ras_x.fits"), 0)


# ------------------------------------------------------------------------------------------------------ SPICE (P9)
def test_spice_preparation_equals_golden(tmp_path):
    arr, meta = Cs.golden()
    c = meta["cases"]["e"]
    A, _ = Cs.make("e", tmp_path)
    assert A.data_small.dtype == np.float64 and A.data_small.shape == (62, 24)
    assert np.array_equal(A.data_small, arr["e/data_small"], equal_nan=True)
    want = c["hdr_small_consumed"]
    for k in ("CDELT1", "CDELT2"):
        print(k, A.hdr_small[k], want[k])
        assert abs(A.hdr_small[k] - want[k]) <= 1e-15 * abs(want[k])
    for k in ("CUNIT1", "CUNIT2", "DATE-AVG"):
        assert str(A.hdr_small[k]).strip() == want[k]
    assert np.array_equal(A.data_large, arr["e/large"].astype(np.float64))


def test_align_pixels_shift_equals_golden(tmp_path):
    _, meta = Cs.golden()
    c = meta["cases"]["e"]
    g = c["align_pixels_shift"]
    assert "header" in g, g
    p_fsi, p_spice = Cs.write_spice(tmp_path)
    hdr = align_pixels_shift(g["delta_pix1"], g["delta_pix2"], g["windows"], p_fsi, c["fsi_window"], p_spice)
    for k, v in g["header"].items():
        print(k, hdr[k], v)
        assert abs(hdr[k] - v) <= 1e-12 * max(1.0, abs(v))
    assert fits_io.read_header(p_spice, 0)["CRVAL1"] != hdr["CRVAL1"]  # (the file is not touched)
