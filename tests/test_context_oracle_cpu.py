"""CPU tests of the iterative-context oracle (oracle/context_oracle.py), the yardstick of tests/test_gpu_context_fuzz.py:
it reproduces the reference-run fixture (tests/golden/iterative_context_golden), and the headers it composes from the
reference's rules equal the library's host planning (coreg_context_lag_headers) bit for bit."""
import struct

import numpy as np
import pytest

from oracle import context_oracle as CO
from tests import context_cases as CC
from tests.test_iterative_context_cpu import cases, load, prepared


@pytest.mark.parametrize("cname", cases())
def test_oracle_reproduces_the_reference_run(cname, tmp_path):
    from euispice_coreg_amd.utils import fits_io
    g, m = load()
    case = m["cases"][cname]
    A, target, headers, cf = prepared(case["window"], tmp_path, case["lags_arcsec"])
    frames = [np.asarray(fits_io.read_image(p, -1)[0]) for p in A.large_fov_list_paths]
    got = CO.context_sweep(frames, headers, cf, np.asarray(A.data_small, dtype=np.float64), target, A.hdr_small,
                           (A.lag_crval1, A.lag_crval2, A.lag_cdelt1, A.lag_cdelt2, A.lag_crota), method=case["method"],
                           semantics=CO.REFERENCE, vmin=case["small_fov_value_min"], vmax=case["small_fov_value_max"])
    want = g[f"{cname}/corr"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-7, np.nanmax(np.abs(got - want))


def _bits(v):
    return struct.pack("<d", float(v))


FIELDS = ("CRPIX1", "CRPIX2", "CRVAL1", "CRVAL2", "CDELT1", "CDELT2", "PC1_1", "PC1_2", "PC2_1", "PC2_2", "CROTA",
          "LONPOLE", "NAXIS1", "NAXIS2")


def _scenes(tmp_path):
    """(target4, hdr_small) pairs: the fixture's window P05 and synthetic rasters (rotated, negative CDELT1, CRPIX off
    centre, a target CRPIX a quarter pixel away)."""
    A, target, _, _ = prepared("P05", tmp_path, [[0.0], [0.0], None, None, None])
    out = [(target, dict(A.hdr_small))]
    for seed in (3, 11, 23, 31):
        c = CC.make_case(seed)
        out.append((c["target4"], c["hdr_small"]))
    return out


@pytest.mark.parametrize("semantics", [CO.INTENDED, CO.REFERENCE])
def test_oracle_headers_equal_the_library_s_bit_for_bit(semantics, tmp_path):
    from euispice_coreg_amd import _lib
    sem = _lib.CDELT_INTENDED if semantics == CO.INTENDED else _lib.CDELT_REFERENCE
    rng = np.random.default_rng(7)
    checked = none = 0
    for target, small in _scenes(tmp_path):
        cd1, cd2 = abs(float(small["CDELT1"])), abs(float(small["CDELT2"]))
        for k in range(80):
            lag = [rng.uniform(-20, 20) * CC.AS, rng.uniform(-20, 20) * CC.AS,
                   rng.uniform(-0.3, 0.3) * cd1, rng.uniform(-0.3, 0.3) * cd2, rng.uniform(-5, 5)]
            for j in range(5):  # each axis exactly zero a good part of the time
                if rng.random() < 0.4:
                    lag[j] = 0.0
            if k == 0:
                lag[2] = -float(small["CDELT1"])  # CDELT1 + lag = 0: no header (intended semantics)
            want = _lib.context_lag_headers(target, small, *lag, cdelt_semantics=sem)
            got = CO.lag_headers(target, small, *lag, semantics=semantics)
            assert (got is None) == (want is None), (lag, semantics)
            if got is None:
                none += 1
                continue
            for g, w in zip(got, want):
                wd = _lib.wcs_to_dict(w)
                for f in FIELDS:
                    assert _bits(g[f]) == _bits(wd[f]), (f, g[f], wd[f], lag, semantics)
            checked += 1
    assert checked >= 120 and none >= 5, (checked, none)
