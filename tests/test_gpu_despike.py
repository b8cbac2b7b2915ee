"""
GPU tests of the median/MAD despiking (coreg_despike_small, coreg_set_reference_despike, coreg_pixels_despike_*) against
tests/despike_oracle.py, the rule in numpy.  The rule is selection, comparison and four separately rounded float64
operations, so every pixel-level comparison is an equality: np.array_equal(..., equal_nan=True), with equal counts per
pass.  The shapes are those at which a tiled window kernel goes wrong: images smaller than a window, one row, one column,
one pixel past the kernel's tile in both axes (taken from csrc/despike_plan.hpp).
"""
import numpy as np
import pytest

from tests import despike_oracle as DO
from tests import helpers as H
from tests.despike_cases import TILE_H, TILE_W, image, rule

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 40), (40, 1), (5, 7), (TILE_H + 1, TILE_W + 1)]


def holes(v, kind):
    v = v.copy()
    ny, nx = v.shape
    if kind == "block":  # wider than any window: pixels inside see no neighbour, pixels at its rim a clipped set
        v[ny // 4:ny // 4 + 8, nx // 4:nx // 4 + 9] = np.nan
    elif kind == "row":
        v[ny // 2, :] = np.nan
    elif kind == "inf":
        v[ny // 3, nx // 2] = np.inf
        v[ny // 2, nx // 4] = -np.inf
        v[0, nx - 1] = np.inf
    elif kind == "all_nan":
        v[:] = np.nan
    return v


def check_all_three(h, v, what, **prm):
    """coreg_despike_small (the image keeps its dtype), coreg_pixels_despike_large and _small (float64 images) against the
    oracle, bit for bit, with equal counts per pass."""
    want, want_counts = DO.despike(v, **prm)
    h.set_small(v)
    counts = h.despike_small(prm)
    got = h.get_small(v.shape, v.dtype)
    assert counts == want_counts, f"{what}: despike_small flagged {counts}, the oracle {want_counts}"
    assert got.dtype == v.dtype and np.array_equal(got, want, equal_nan=True), f"{what}: despike_small differs"
    v64 = v.astype(np.float64)
    want64, want_counts64 = (want, want_counts) if v.dtype == np.float64 else DO.despike(v64, **prm)
    flipped = v64[::-1].copy()
    want_f, want_counts_f = DO.despike(flipped, **prm)
    h.pixels_set_large(v)
    h.pixels_set_small(flipped)
    counts_l = h.pixels_despike_large(prm)
    counts_s = h.pixels_despike_small(prm)
    assert counts_l == want_counts64 and counts_s == want_counts_f, f"{what}: pixels counts {counts_l} {counts_s}"
    assert np.array_equal(h.pixels_get_image("large", v.shape), want64, equal_nan=True), f"{what}: pixels_despike_large"
    assert np.array_equal(h.pixels_get_image("small", v.shape), want_f, equal_nan=True), f"{what}: pixels_despike_small"
    return want_counts


# ---- 1. the kernels against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_despike_against_the_oracle(gpu_handle, shape, R, dtype):
    flagged = 0
    for n_iter in (1, 3):
        v = image(shape, 3 + R + 7 * n_iter, dtype)
        flagged += sum(check_all_three(gpu_handle, v, f"{shape} R={R} n_iter={n_iter}", **rule(R, n_iter, shape)))
        flagged += sum(check_all_three(gpu_handle, v, f"{shape} R={R} n_iter={n_iter} both/median/floor",
                                       **rule(R, n_iter, shape, sign="both", replace="median", floor=0.75, nsigma=3.0)))
    if shape[0] * shape[1] >= 35:
        assert flagged > 0  # the cases decide both ways


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,hole", [("integers", None), ("integers", "row"), ("constant", None), ("noise", "block"),
                                       ("noise", "row"), ("noise", "inf"), ("noise", "all_nan"), ("integers", "inf")])
def test_despike_ties_holes_and_infinities(gpu_handle, kind, hole, dtype):
    """Integer-valued images (ties, half-integer medians), a constant image, a NaN block wider than the window, a NaN row,
    Inf pixels (never neighbours, never changed), an all-NaN image: a shape of several tiles, ragged in both axes."""
    shape = (2 * TILE_H + 3, TILE_W + 5)
    v = holes(image(shape, 17, dtype, kind), hole)
    for R in (1, 2, 3):
        counts = check_all_three(gpu_handle, v, f"{kind}/{hole} R={R}", **rule(R, 2, sign="both", floor=0.5 if kind == "integers" else 0.0))
        if kind == "constant" or hole == "all_nan":
            assert counts == [0, 0]
    check_all_three(gpu_handle, v, f"{kind}/{hole} median", **rule(2, 3, replace="median"))
    if hole == "inf":
        gpu_handle.set_small(v)
        gpu_handle.despike_small(rule(2, 2, sign="both"))
        got = gpu_handle.get_small(v.shape, v.dtype)
        assert np.array_equal(np.isinf(got), np.isinf(v)) and np.array_equal(got[np.isinf(v)], v[np.isinf(v)])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_seeded_scene_on_the_device(gpu_handle, dtype):
    """The scene of tests/test_despike_cpu.py with the defaults: the oracle's image and counts, bit for bit."""
    from euispice_coreg_amd.utils.despiking import despike_params
    img, truth, raised = DO.scene(dtype)
    counts = check_all_three(gpu_handle, img, "scene", **despike_params(True))
    assert counts[0] >= raised.sum()
    got = gpu_handle.pixels_get_image("large", img.shape)
    assert DO.pearson(img, truth) < 0.5 and DO.pearson(got, truth) > 0.95


def test_min_neighbours_on_the_device(gpu_handle):
    v = np.full((7, 7), np.nan)
    v[3, 3] = 1000.0
    v[3, 4], v[2, 3], v[4, 4], v[3, 1] = 1.0, 2.0, 3.0, 2.5
    assert check_all_three(gpu_handle, v, "four neighbours, five asked", radius=2, n_iter=1, min_neighbours=5) == [0]
    assert check_all_three(gpu_handle, v, "four neighbours, four asked", radius=2, n_iter=1, min_neighbours=4) == [1]


def spiked(v, seed, n=None, lo=300.0, hi=5000.0):
    """`v` with n (default: 1 in 60 pixels) seeded pixels raised by uniform(lo, hi), a third of them with their right-hand
    neighbour raised too; the pixels stay float32-exact where they were."""
    rng = np.random.default_rng(seed)
    out = np.array(v, copy=True)
    ny, nx = out.shape
    n = max(4, out.size // 60) if n is None else n
    flat = rng.choice(ny * (nx - 1), size=n, replace=False)
    jj, ii = flat // (nx - 1), flat % (nx - 1)
    out[jj, ii] += np.round(rng.uniform(lo, hi, n))
    out[jj[:n // 3], ii[:n // 3] + 1] += 800.0
    return out.astype(np.float32).astype(out.dtype)


# ---- 2. the reference image -----------------------------------------------------------------------------------------------
SHAPE = (48, 40)
SMALL_GRID = ((244.0, 246.5), (3.0, 5.0), (40, 50))  # touches a small part of the image: the crop is taken
REF_RULE = dict(radius=3, n_iter=2, nsigma=4.0, min_neighbours=5, sign="both", replace="median", floor=0.0)


def _references(h, hs, prepare_c, prepare_h):
    """[crop on, crop off] x [the usual Carrington grid, a small one, helioprojective] of the prepared reference, and the
    counts of the last preparation per crop setting."""
    from euispice_coreg_amd import _lib
    out, counts = [], []
    for crop in (1, 0):
        h.set_option("crop_reference", crop)
        try:
            got = []
            for lon, lat, shape in ((H.CARR_LON, H.CARR_LAT, SHAPE), SMALL_GRID):
                grid = _lib.Grid(lon, lat, shape)
                prepare_c(grid)
                got.append(h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64))
            prepare_h()
            got.append(h.get_reference_on_grid((hs["NAXIS2"], hs["NAXIS1"]), np.float32))
            out.append(got)
            counts.append(h.last_reference_despike())
        finally:
            h.set_option("crop_reference", 1)
    return out, counts


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("smoothing", [False, True])
@pytest.mark.parametrize("f32", [True, False])
def test_reference_despike_equals_the_preparation_of_the_oracle_despiked_image(gpu_handle, tmp_path, f32, smoothing):
    """coreg_set_reference_despike: the prepared reference is, bit for bit, what the library prepares from the
    oracle-despiked image -- with "crop_reference" 1 and 0 (the crop box is widened by n_iter * radius, plus the reach of
    the reference smoothing when that is set too), on a Carrington grid that touches a small part of the image and on the
    helioprojective frame, from host, FITS and device sources; the device source is not modified."""
    import torch
    from euispice_coreg_amd.utils import fits_io
    h = gpu_handle
    small, hs, large, hl, _ = H.scene(small_n=40, large_n=160)
    large = spiked(large, 23)
    large = large.astype(np.float32) if f32 else large + 1e-9 * np.arange(large.size).reshape(large.shape)
    large[70:73, 60:90] = np.nan
    want_img, want_counts = DO.despike(large, **REF_RULE)
    assert want_counts[0] > 50 and not np.array_equal(want_img, large, equal_nan=True)
    tables = (np.array([0.2, 0.5, 0.3]), np.array([0.1, 0.2, 0.4, 0.2, 0.1])) if smoothing else None

    def host(img):
        return _references(h, hs, lambda g: h.prepare_reference_carrington(img, hl, g, 1.004, 2),
                           lambda: h.prepare_reference_helioprojective(img, hl, hs, 2))
    h.set_small(small)
    try:
        h.set_reference_smoothing(tables)
        h.set_reference_despike(None)
        want, none = host(want_img)
        assert none == [[0] * 8, [0] * 8]
        spiky, _ = host(large)
        assert not any(np.array_equal(a, b, equal_nan=True) for a, b in zip(want[0], spiky[0]))
        assert _same(want[0], want[1])
        h.set_reference_despike(REF_RULE)
        got, counts = host(large)
        assert _same(got[0], want[0]) and _same(got[1], want[0])
        assert counts[1] == want_counts + [0] * 6  # crop off: the whole image was processed
        assert counts[0][0] > 0 and counts[0][2:] == [0] * 6  # crop on: the pixels of the box alone
        # device source: not modified, same bits
        t = torch.from_numpy(np.ascontiguousarray(large)).cuda()
        torch.cuda.synchronize()
        dev, _ = _references(h, hs,
                             lambda g: h.prepare_reference_carrington_from_device(t.data_ptr(), t.shape, large.dtype, hl, g, 1.004, 2),
                             lambda: h.prepare_reference_helioprojective_from_device(t.data_ptr(), t.shape, large.dtype, hl, hs, 2))
        h.synchronize()
        assert np.array_equal(t.cpu().numpy(), large, equal_nan=True)
        # FITS data unit, decoded on the GPU
        path = str(tmp_path / "l.fits")
        fits_io.write_images(path, [(None, {}), (large, dict(hl))])
        raw = fits_io.open_raw(path, -1)
        assert raw is not None
        fits, _ = host(raw)
        for other in (dev, fits):
            assert _same(other[0], want[0]) and _same(other[1], want[0])
    finally:
        h.set_reference_despike(None)
        h.set_reference_smoothing(None)


def test_reference_despike_of_a_tile_compressed_source(gpu_handle, tmp_path):
    """The same from a tile-compressed image, whose pixels are decoded on the GPU (lossless 16-bit integers)."""
    from euispice_coreg_amd.utils import fits_io
    h = gpu_handle
    small, hs, large, hl, _ = H.scene(small_n=40, large_n=160)
    img = np.clip(np.nan_to_num(spiked(large, 29), nan=0.0), 0, 65535).astype(np.uint16)
    path = str(tmp_path / "c.fits")
    fits_io.write_compressed_image(path, img, hl)
    ci = fits_io.open_compressed(path, -1)
    assert ci.on_gpu
    decoded = fits_io.native_pixels(ci.decode())
    prm = dict(REF_RULE, replace="nan")
    want_img, want_counts = DO.despike(np.asarray(decoded, dtype=np.float64), **prm)
    assert want_counts[0] > 50

    def both(src):
        return _references(h, hs, lambda g: h.prepare_reference_carrington(src, hl, g, 1.004, 2),
                           lambda: h.prepare_reference_helioprojective(src, hl, hs, 2))
    h.set_small(small)
    try:
        h.set_reference_despike(None)
        want, _ = both(fits_io.native_pixels(want_img))
        h.set_reference_despike(prm)
        got, counts = both(ci)
        assert _same(got[0], want[0]) and _same(got[1], want[0])
        assert counts[0][:2] == want_counts and counts[1][:2] == want_counts  # a decoded image is processed whole
    finally:
        h.set_reference_despike(None)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
BAD_RULES = [dict(radius=0), dict(radius=4), dict(n_iter=0), dict(n_iter=9), dict(nsigma=0.0), dict(nsigma=-1.0),
             dict(nsigma=float("nan")), dict(nsigma=float("inf")), dict(floor=-1.0), dict(floor=float("nan")),
             dict(floor=float("inf")), dict(min_neighbours=0), dict(min_neighbours=25), dict(radius=1, min_neighbours=9),
             dict(radius=3, min_neighbours=49), dict(sign=2), dict(sign=-1), dict(replace=2), dict(replace=-1)]


def test_refusals_by_error_code_and_state_kept(gpu_handle):
    from euispice_coreg_amd import _lib
    with _lib.CoregHandle(0) as fresh:  # no image
        for call in (fresh.despike_small, fresh.pixels_despike_large, fresh.pixels_despike_small):
            with pytest.raises(_lib.CoregError) as e:
                call({})
            assert e.value.code == _lib.COREG_ESTATE
        assert fresh.last_reference_despike() == [0] * 8
        fresh.set_reference_despike({})
        fresh.set_reference_despike(None)
    h = gpu_handle
    v = spiked(image((37, 45), 2, np.float32), 4)
    h.set_small(v)
    h.pixels_set_large(v)
    h.pixels_set_small(v[::-1].copy())
    small, hs, large, hl, _ = H.scene(small_n=40, large_n=160)
    large = spiked(large, 23)
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, SHAPE)

    def ref():
        h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        return h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64)
    try:
        h.set_reference_despike(None)
        plain = ref()
        h.set_reference_despike(REF_RULE)
        despiked = ref()
        assert not np.array_equal(plain, despiked, equal_nan=True)
        for bad in BAD_RULES:
            for call in (h.despike_small, h.pixels_despike_large, h.pixels_despike_small, h.set_reference_despike):
                with pytest.raises(_lib.CoregError) as e:
                    call(bad)
                assert e.value.code == _lib.COREG_EINVAL, (bad, call)
        # the images are as they were, float32 where they were ...
        assert np.array_equal(h.get_small(v.shape, np.float32), v, equal_nan=True)
        assert np.array_equal(h.pixels_get_image("large", v.shape), v.astype(np.float64), equal_nan=True)
        assert np.array_equal(h.pixels_get_image("small", v.shape), v[::-1].astype(np.float64), equal_nan=True)
        # ... and so are the earlier parameters of the reference despiking; clearing them restores the plain reference
        assert np.array_equal(ref(), despiked, equal_nan=True)
        h.set_reference_despike(None)
        assert np.array_equal(ref(), plain, equal_nan=True)
    finally:
        h.set_reference_despike(None)


# ---- 4. maps ------------------------------------------------------------------------------------------------------------------
MAP_RULE = dict(radius=2, n_iter=2, nsigma=5.0, min_neighbours=5, sign="positive", replace="nan", floor=0.0)


@pytest.fixture(scope="module")
def maps():
    """The usual scene with spikes added to both images, 5 x 5 CRVAL lags, and both images despiked by the oracle, once."""
    from tests.test_gpu_masked_scores import _lags
    small, hs, large, hl, _ = H.scene()
    small, large = spiked(small, 31), spiked(large, 37)
    small_d, counts_s = DO.despike(small, **MAP_RULE)
    large_d, counts_l = DO.despike(large, **MAP_RULE)
    assert counts_s[0] > 100 and counts_l[0] > 300
    return dict(small=small, hs=hs, large=large, hl=hl, lags=_lags(5, 5), small_d=small_d, large_d=large_d,
                counts_s=counts_s, counts_l=counts_l)


def _on_device(h, m, grid=None, order=2, frame="carrington"):
    """Both spiked images up and despiked on the device, the reference prepared from the despiked large image."""
    h.set_reference_despike(MAP_RULE)
    try:
        h.set_small(m["small"])
        assert h.despike_small(MAP_RULE) == m["counts_s"]
        if frame == "carrington":
            h.prepare_reference_carrington(m["large"], m["hl"], grid, 1.004, order)
        else:
            h.prepare_reference_helioprojective(m["large"], m["hl"], m["hs"], order)
    finally:
        h.set_reference_despike(None)


def _from_arrays(h, m, grid=None, order=2, frame="carrington", despiked=True):
    """The oracle-despiked (or the spiked) arrays handed to the library."""
    h.set_reference_despike(None)
    h.set_small(m["small_d"] if despiked else m["small"])
    large = m["large_d"] if despiked else m["large"]
    if frame == "carrington":
        h.prepare_reference_carrington(large, m["hl"], grid, 1.004, order)
    else:
        h.prepare_reference_helioprojective(large, m["hl"], m["hs"], order)


@pytest.mark.parametrize("order", [1, 2])
def test_carrington_map_of_device_despiked_images(gpu_handle, maps, order):
    from euispice_coreg_amd import _lib
    m, h = maps, gpu_handle
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    ls = _lib.LagSet(*m["lags"])
    _from_arrays(h, m, grid, order)
    ref = h.sweep_carrington(m["hs"], grid, 1.004, ls, order=order)
    ref_counts = h.last_counts()
    _on_device(h, m, grid, order)
    got = h.sweep_carrington(m["hs"], grid, 1.004, ls, order=order)
    assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(h.last_counts(), ref_counts, equal_nan=True)
    want = H.oracle_carrington(m["small_d"], m["hs"], m["large_d"], m["hl"], m["lags"], (48, 40), order=order)
    H.assert_corr_close(got.reshape(want.shape), want, 1e-10, f"carrington, order {order}")
    assert np.nanargmax(got) == np.nanargmax(want) and np.isfinite(want).all()
    _from_arrays(h, m, grid, order, despiked=False)
    spiky = h.sweep_carrington(m["hs"], grid, 1.004, ls, order=order)
    assert np.nanmax(np.abs(spiky - got)) > 1e-3


@pytest.mark.parametrize("order", [1, 2])
def test_helioprojective_map_of_device_despiked_images(gpu_handle, maps, order):
    from euispice_coreg_amd import _lib
    m, h = maps, gpu_handle
    ls = _lib.LagSet(*m["lags"])
    _from_arrays(h, m, order=order, frame="helioprojective")
    ref = h.sweep_helioprojective(m["hs"], m["hs"], ls, order=order)
    ref_counts = h.last_counts()
    _on_device(h, m, order=order, frame="helioprojective")
    got = h.sweep_helioprojective(m["hs"], m["hs"], ls, order=order)
    assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(h.last_counts(), ref_counts, equal_nan=True)
    want = H.oracle_helio(m["small_d"], m["hs"], m["large_d"], m["hl"], m["lags"], order=order)
    H.assert_corr_close(got.reshape(want.shape), want, 1e-7, f"helioprojective, order {order}")
    assert np.nanargmax(got) == np.nanargmax(want)
    _from_arrays(h, m, order=order, frame="helioprojective", despiked=False)
    spiky = h.sweep_helioprojective(m["hs"], m["hs"], ls, order=order)
    assert np.nanmax(np.abs(spiky - got)) > 1e-3


def test_masked_residus_and_mutual_information_of_device_despiked_images(gpu_handle, maps):
    """Masked residus and mutual information: the device-despiked images against the oracle-despiked arrays handed to
    the library, bit for bit (mutual information with default bins, the quantiles of the images as the sweep sees them),
    and against the CPU oracles with their usual bounds (mutual information with quantile edges that keep tests/
    test_gpu_hdrshift_mi.py's precondition: no kept value within 1e-8, relative, of an edge)."""
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.hdrshift.alignment import default_edges
    from euispice_coreg_amd.pxlshift.alignment_pixels import quantile_edges
    from oracle import coreg_oracle as O
    from tests import hdrshift_mi_oracle as MO
    from tests import masked_scores_oracle as M
    from tests.test_gpu_hdrshift_mi import BOUND_MARGIN, EDGE_MARGIN, _check
    from tests.test_gpu_masked_scores import CARR_RTOL, assert_counts, assert_masked, carr_state
    m, h = maps, gpu_handle
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    ls = _lib.LagSet(*m["lags"])

    def state():
        return carr_state(m["small_d"], m["hs"], m["large_d"], m["hl"], m["lags"], (48, 40))
    want = M.sweep(state(), "carrington")
    _from_arrays(h, m, grid)
    ref = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_RESIDUS_MASKED)
    ref_counts = h.last_counts()
    # default bins: the quantiles of the images as the sweep sees them (what hdrshift.Alignment hands the library)
    es, el = default_edges(h.get_small(m["small"].shape), None, None, h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64), 16)
    h.sweep_set_bins(es, el)
    ref_mi = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_MUTUAL_INFORMATION)
    ref_mi_counts = h.last_counts()
    _on_device(h, m, grid)
    got = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_RESIDUS_MASKED)
    assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(h.last_counts(), ref_counts, equal_nan=True)
    assert_counts(h.last_counts(), want["finite_terms"], "despiked, masked")
    assert_masked(got, want["masked"], CARR_RTOL, "despiked, masked residus")
    es2, el2 = default_edges(h.get_small(m["small"].shape), None, None, h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64), 16)
    assert np.array_equal(es, es2) and np.array_equal(el, el2)
    h.sweep_set_bins(es, el)
    got_mi = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_MUTUAL_INFORMATION)
    assert np.array_equal(got_mi, ref_mi, equal_nan=True) and np.array_equal(h.last_counts(), ref_mi_counts, equal_nan=True)
    ref_img = O.prepare_reference(state(), "carrington", 1.004, True)
    for n_bins in (8, 7, 9, 6, 10):
        qs, ql = quantile_edges(m["small_d"], n_bins), quantile_edges(ref_img, n_bins)
        edge, bound = MO.margins(state(), qs, ql)
        if edge > EDGE_MARGIN and bound > BOUND_MARGIN:
            break
    print(f"[despike mi] {n_bins} bins: distance to an edge {edge:.2e}, to a bound {bound:.2e} px")
    assert edge > EDGE_MARGIN and bound > BOUND_MARGIN
    want_mi = {k: v.ravel() for k, v in MO.sweep(state(), "carrington", qs, ql).items()}
    h.sweep_set_bins(qs, ql)
    got_q = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_MUTUAL_INFORMATION)
    _check(got_q, h.last_counts(), want_mi, "despiked, mutual information")
    _from_arrays(h, m, grid, despiked=False)
    spiky = h.sweep_carrington(m["hs"], grid, 1.004, ls, method=_lib.METHOD_RESIDUS_MASKED)
    assert not np.array_equal(spiky, got, equal_nan=True)


# ---- 5. the order of thresholds and despiking ------------------------------------------------------------------------------
def saturated_patch():
    """Unit noise about 100, a 7 x 6 saturated patch, and in the middle of its right-hand edge a pixel at 200.  Thresholds
    first: the patch is NaN and the pixel a spike among the neighbours it has left.  Despiking first: the patch is most of
    the pixel's window, the median is the saturation level and the pixel is kept -- and the patch, too wide to be a spike,
    falls to the threshold afterwards."""
    v = (100.0 + np.random.default_rng(8).normal(0.0, 1.0, (21, 23))).astype(np.float32)
    v[7:14, 8:14] = 60000.0
    v[10, 13] = 200.0
    return v, 20000.0, (10, 13)


def test_despiking_follows_the_thresholds(gpu_handle):
    from euispice_coreg_amd.utils import header as hdrutil
    h = gpu_handle
    v, vmax, at = saturated_patch()
    first = v.astype(np.float64)
    hdrutil.set_threshold_minmax_to_nan(first, None, vmax)
    threshold_then_despike, counts = DO.despike(first.astype(np.float32), **MAP_RULE)
    despike_then_threshold, _ = DO.despike(v, **MAP_RULE)
    despike_then_threshold = despike_then_threshold.astype(np.float64)
    hdrutil.set_threshold_minmax_to_nan(despike_then_threshold, None, vmax)
    assert np.isnan(threshold_then_despike[at]) and despike_then_threshold[at] == 200.0  # the constructed pixel
    h.set_small(v)
    h.threshold_small(None, vmax)
    assert h.despike_small(MAP_RULE) == counts
    assert np.array_equal(h.get_small(v.shape, np.float32), threshold_then_despike, equal_nan=True)
    h.set_small(v)
    h.despike_small(MAP_RULE)
    h.threshold_small(None, vmax)
    assert np.array_equal(h.get_small(v.shape), despike_then_threshold, equal_nan=True)


# ---- 6. several devices -----------------------------------------------------------------------------------------------------
def test_multi_handle_on_one_gpu_equals_the_single_handle(gpu_handle, maps, monkeypatch):
    from euispice_coreg_amd import _lib
    monkeypatch.setenv("COREG_VIRTUAL_DEVICES", "2")
    m, h = maps, gpu_handle
    grid = _lib.Grid(H.CARR_LON, H.CARR_LAT, (48, 40))
    ls = _lib.LagSet(*m["lags"])
    _on_device(h, m, grid)
    want = h.sweep_carrington(m["hs"], grid, 1.004, ls)
    want_small = h.get_small(m["small"].shape)
    want_ref = h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64)
    want_counts = h.last_reference_despike()
    with _lib.MultiHandle() as mh:
        assert mh.size == 2
        _on_device(mh, m, grid)
        got = mh.sweep_carrington(m["hs"], grid, 1.004, ls)
        assert np.array_equal(mh.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64), want_ref, equal_nan=True)
        assert mh.last_reference_despike() == want_counts
        for k in range(mh.size):  # every device holds the despiked image
            assert np.array_equal(mh.handle(k).get_small(m["small"].shape), want_small, equal_nan=True)
        with pytest.raises(_lib.CoregError) as e:
            mh.despike_small(dict(radius=7))
        assert e.value.code == _lib.COREG_EINVAL
        with pytest.raises(_lib.CoregError) as e:
            mh.set_reference_despike(dict(n_iter=0))
        assert e.value.code == _lib.COREG_EINVAL
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-12 and np.nanargmax(got) == np.nanargmax(want)  # (tests/test_gpu_multi.py)


# ---- 7. end to end, on files ------------------------------------------------------------------------------------------------
RESOLVED_GRID = ((243.5, 246.5), (3.5, 6.5), (48, 40))


def resolved_scene():
    """A 64 x 64 field of 2 arcsec pixels inside a 128 x 128 reference image of 4.44 arcsec pixels: the structures span
    several pixels of either image, as real ones do, so that a spike is what stands alone (in the usual test scene of 10
    arcsec pixels most structures are narrower than a pixel and the rule takes the brightest of them for spikes).
    RESOLVED_GRID lies inside the field.  The CPU oracle's helioprojective map of the pair used below: peak 0.999 at the
    injected lag without spikes, 0.868 one lag off with them, 0.994 at the injected lag after the oracle's despiking."""
    return H.scene(small_n=64, large_n=128, small_cdelt=(2.0, 2.0), large_cdelt=4.44, large_crval=(-300.0, 410.0))


@pytest.fixture()
def whole_reference():
    """The classes' shared handle with "crop_reference" off, so that the counts of the reference image cover all of it and
    can be held to the oracle's (the pixels are the same either way: see the crop tests above)."""
    from euispice_coreg_amd import _lib
    h = _lib.shared_handle(-1)
    h.set_option("crop_reference", 0)
    yield h
    h.set_option("crop_reference", 1)


def test_alignment_applies_both_keywords_on_every_path(tmp_path, whole_reference):
    """hdrshift.Alignment with despike_small and despike_large on FITS files against the oracle fed the oracle-despiked
    arrays: the Carrington frame, the helioprojective frame with parallelism True (sub-map) and False (the reference image
    despiked on its own grid), the thresholds applied before the despiking; `last_despiked` holds the oracle's counts; on
    the spiked pair the injected lag is the best entry with the keywords, and without them the peak is lower; default
    mutual-information bins are the quantiles of the despiked images; the handle keeps no reference despiking."""
    from euispice_coreg_amd import _lib
    from euispice_coreg_amd.hdrshift import Alignment
    from euispice_coreg_amd.hdrshift.alignment import default_edges
    from euispice_coreg_amd.utils import fits_io, header as hdrutil
    from oracle import coreg_oracle as O
    from tests.test_gpu_masked_scores import _lags, carr_state
    small, hs, large, hl, _ = resolved_scene()
    small, large = spiked(small, 41).astype(np.float32), spiked(large, 43).astype(np.float32)
    ps, pl = str(tmp_path / "small.fits"), str(tmp_path / "large.fits")
    fits_io.write_images(ps, [(None, {}), (small, hs)])
    fits_io.write_images(pl, [(None, {}), (large, hl)])
    lag1, lag2 = _lags(5, 5)[:2]
    lon, lat, shape = RESOLVED_GRID
    lags = (lag1, lag2, None, None, None)
    vmax = 4000.0
    host = small.astype(np.float64)
    hdrutil.set_threshold_minmax_to_nan(host, None, vmax)
    assert np.isnan(host).sum() > np.isnan(small).sum()
    small_d, counts_s = DO.despike(host.astype(np.float32), **MAP_RULE)
    large_d, counts_l = DO.despike(large, **MAP_RULE)
    small_d, large_d = small_d.astype(np.float64), large_d.astype(np.float64)
    assert counts_s[0] > 30 and counts_l[0] > 60
    kw = dict(small_fov_value_max=vmax, despike_small=MAP_RULE, despike_large=True)
    ckw = dict(lonlims=lon, latlims=lat, shape=shape, return_type="corr")
    A = Alignment(pl, ps, lag1, lag2, None, None, None, **kw)
    got = A.align_using_carrington(**ckw)
    want = H.oracle_carrington(small_d, hs, large_d, hl, lags, shape, lon, lat)
    H.assert_corr_close(got, want, 1e-10, "class, carrington")
    assert A.last_despiked == {"small": counts_s, "large": counts_l}
    assert np.unravel_index(np.nanargmax(got), got.shape)[:2] == (2, 2)  # the injected lag
    plain = Alignment(pl, ps, lag1, lag2, None, None, None, small_fov_value_max=vmax)
    spiky = plain.align_using_carrington(**ckw)
    assert plain.last_despiked is None or plain.last_despiked == {"small": [], "large": []}
    print(f"[despike] carrington peak {np.nanmax(spiky):.4f} without, {np.nanmax(got):.4f} with the keywords")
    assert np.nanmax(spiky) < np.nanmax(got)
    for parallelism in (True, False):
        A = Alignment(pl, ps, lag1, lag2, None, None, None, parallelism=parallelism, **kw)
        got = A.align_using_helioprojective(return_type="corr")
        want = H.oracle_helio(small_d, hs, large_d, hl, lags, parallelism=parallelism)
        H.assert_corr_close(got, want, 1e-7, f"class, helioprojective, parallelism={parallelism}")
        assert A.last_despiked == {"small": counts_s, "large": counts_l}, parallelism
    # default mutual-information bins: the quantiles of the images as the sweep sees them
    A = Alignment(pl, ps, lag1, lag2, None, None, None, **kw)
    got = A.align_using_carrington(**ckw, method="mutual_information", bins=8)
    ref = O.prepare_reference(carr_state(small_d, hs, large_d, hl, _lags(1, 1), shape, lon, lat), "carrington", 1.004, True)
    es, el = default_edges(small_d, None, None, ref, 8)
    assert np.allclose(A.last_bins[0], es, rtol=1e-12, atol=0) and np.allclose(A.last_bins[1], el, rtol=1e-10, atol=0)
    assert np.isfinite(got).all()
    # the handle the classes ran on does not keep the reference despiking
    h = whole_reference
    grid = _lib.Grid(lon, lat, shape)
    h.prepare_reference_carrington(large, hl, grid, 1.004, 2)
    after = h.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64)
    assert h.last_reference_despike() == [0] * 8
    with _lib.CoregHandle(0) as fresh:
        fresh.prepare_reference_carrington(large, hl, grid, 1.004, 2)
        assert np.array_equal(fresh.get_reference_on_grid((grid.n_lat, grid.n_lon), np.float64), after, equal_nan=True)


def test_alignment_spice_despikes_the_summed_image(whole_reference):
    """AlignmentSpice: the step acts on the 2-D image after the wavelength sum, the slit-edge mask and the thresholds."""
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.hdrshift import AlignmentSpice
    cube, h4, large, hl, truth = synthetic.make_spice_l2()
    cube = np.array(cube, copy=True)
    plane = cube.shape[1] // 2
    cube[0, plane] = spiked(cube[0, plane], 47, n=60, lo=200.0, hi=3000.0)  # hits that survive the sum over the planes
    large = spiked(large, 53)
    lag1, lag2 = np.arange(-31.0, -14.0, 4.0), np.arange(28.0, 45.0, 4.0)
    kw = dict(lag_crval1=lag1, lag_crval2=lag2, parallelism=True, level=2)
    A = AlignmentSpice((large, hl), (cube, h4), despike_small=True, despike_large=True, **kw)
    with pytest.warns(UserWarning):
        got = A.align_using_helioprojective(method="correlation", return_type="corr")
    img = np.asarray(A.data_small)
    assert img.ndim == 2 and img.dtype in (np.float32, np.float64)
    small_d, counts_s = DO.despike(img, **DO.DEFAULTS)
    large_d, counts_l = DO.despike(large, **DO.DEFAULTS)
    assert counts_s[0] >= 40 and A.last_despiked == {"small": counts_s, "large": counts_l}
    want = H.oracle_helio(small_d.astype(np.float64), A.hdr_small, large_d, hl, (lag1, lag2, [0.0], [0.0], [0.0]),
                          parallelism=True, unit_lag="arcsec")
    H.assert_corr_close(got, want, 1e-7, "AlignmentSpice with both keywords")
    B = AlignmentSpice((large, hl), (cube, h4), **kw)
    with pytest.warns(UserWarning):
        spiky = B.align_using_helioprojective(method="correlation", return_type="corr")
    print(f"[despike] spice peak {np.nanmax(spiky):.4f} without, {np.nanmax(got):.4f} with the keywords")
    assert np.nanmax(spiky) < np.nanmax(got)
    assert np.unravel_index(np.nanargmax(got), got.shape)[:2] == (list(lag1).index(truth["lag_crval1"]),
                                                                  list(lag2).index(truth["lag_crval2"]))


def test_jitter_session_prepares_the_reference_despiked(tmp_path):
    """jitter_correction_imagers with both keywords: every map is the oracle's for the thresholded, then despiked frame
    against the despiked reference frame."""
    from euispice_coreg_amd import synthetic
    from euispice_coreg_amd.jitter_correction import jitter_correction_imagers
    from euispice_coreg_amd.utils import fits_io
    from oracle import coreg_oracle as O
    frames, jit = synthetic.make_series(n_frames=3, n=128, seed=7, jitter_sigma=2.0)
    frames = [(spiked(img, 60 + k), hdr) for k, (img, hdr) in enumerate(frames)]
    paths = []
    for k, (img, hdr) in enumerate(frames):
        assert img.dtype == np.float32
        p = str(tmp_path / f"solo_L2_eui-hrieuv174-image_{k:03d}.fits")
        fits_io.write_images(p, [(None, {}), (img, hdr)])
        paths.append(p)
    lon, lat, shape = (236.0, 256.0), (-4.0, 16.0), (100, 100)
    lag = np.arange(-4.0, 4.5, 2.0)
    kw = dict(lonlims=lon, latlims=lat, shape=shape, lag_crval1=lag, lag_crval2=lag, sublist_length=3, overlap=1,
              small_fov_value_max=2800.0)
    done = jitter_correction_imagers(paths, str(tmp_path / "out"), despike_small=True, despike_large=True, **kw)
    plain = jitter_correction_imagers(paths, str(tmp_path / "out_plain"), **kw)
    assert [(a, r) for a, r, _ in done] == [(a, r) for a, r, _ in plain] and len(done) == 2
    assert all(r == 0 for _, r, _ in done)  # (frame 0, whose header no correction changes, is the reference of both)
    ref_d = DO.despike(frames[0][0], **DO.DEFAULTS)[0].astype(np.float64)
    for (idx, ref, res), (_, _, res_plain) in zip(done, plain):
        img = frames[idx][0].astype(np.float64)
        O.set_threshold_minmax_to_nan(img, None, 2800.0)
        img_d = DO.despike(img.astype(np.float32), **DO.DEFAULTS)[0].astype(np.float64)
        want = H.oracle_carrington(img_d, frames[idx][1], ref_d, frames[0][1], (lag, lag, [0], [0], [0]), shape, lon, lat)
        H.assert_corr_close(res.corr, want, 1e-10, f"jitter frame {idx} vs {ref}, despiked")
        assert np.nanmax(res_plain.corr) < np.nanmax(res.corr)


@pytest.mark.parametrize("name", ["a"])
def test_pxlshift_despikes_both_images(name, tmp_path):
    """find_best_parameters (correlation, residus_masked) and find_local_shifts with both keywords on a spiked pair of
    files against the oracles fed the oracle-despiked images; `last_despiked` holds the oracle's counts; the best entry is
    that of the pair without spikes and the peak is higher than without the keywords; a later call without the keywords
    starts from the file's pixels again."""
    from euispice_coreg_amd.pxlshift import AlignmentPixels
    from tests import pxlshift_cases as Cs
    from tests import pxlshift_scores_oracle as S
    from tests import pxlshift_tiles_oracle as T
    from tests.test_gpu_pxlshift_scores import _check_corr, _check_masked
    from tests.test_gpu_pxlshift_tiles import TILES, _check, _local
    clean, kw = Cs.make(name, tmp_path)
    clean_cube = clean.find_best_parameters(**kw)
    small, hs, large, hl = Cs.inputs(name)
    small, large = spiked(small, 71), spiked(large, 73)
    sub = tmp_path / "spiked"
    sub.mkdir()
    pl, ps = Cs.write_pair(sub, name, small, hs, large, hl)
    A = AlignmentPixels(pl, 0, ps, 0)
    rule_l, rule_s = dict(MAP_RULE), dict(MAP_RULE, radius=1, n_iter=1)
    large_d, counts_l = DO.despike(np.asarray(A.data_large, dtype=np.float64), **rule_l)
    small_d, counts_s = DO.despike(np.asarray(A.data_small, dtype=np.float64), **rule_s)
    assert counts_l[0] > 0 and counts_s[0] > 0
    plan = A.host_plan(**kw)
    o = S.scores(large_d, small_d, plan)
    both = dict(despike_large=rule_l, despike_small=rule_s)
    corr = A.find_best_parameters(**kw, **both)
    assert A.last_despiked == {"small": counts_s, "large": counts_l}
    assert np.array_equal(A.last_counts, o["count"])
    _check_corr(corr, o["corr"], name + " despiked")
    masked = A.find_best_parameters(**kw, method="residus_masked", **both)
    assert np.array_equal(A.last_counts, o["finite_terms"])
    _check_masked(masked, o["masked"], name + " despiked")
    ot = T.scores(large_d, small_d, plan, TILES[name])
    got, n, _ = _local(A, kw, TILES[name], "correlation", **both)
    assert np.array_equal(n, ot["count"]) and A.last_despiked == {"small": counts_s, "large": counts_l}
    _check(got, ot["corr"], "correlation", name + " despiked tiles", ties=True)
    # what it is for: the best entry of the clean pair, and a higher peak than the spiked pair gives
    spiky = A.find_best_parameters(**kw)
    assert A.last_despiked == {"small": [], "large": []}
    print(f"[despike] pxlshift peak {np.nanmax(spiky):.4f} without, {np.nanmax(corr):.4f} with the keywords")
    assert np.nanargmax(corr) == np.nanargmax(clean_cube) and np.nanmax(spiky) < np.nanmax(corr)
    B = AlignmentPixels(pl, 0, ps, 0)
    assert np.array_equal(B.find_best_parameters(**kw), spiky, equal_nan=True)  # no trace of the despiking
