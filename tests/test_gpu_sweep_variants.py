"""
Every generic k_sweep instantiation against the CPU oracles, with proof of which one ran: one test per row of
tests/sweep_variant_cases.py (frame x spline order x pixel type x method; 84 rows over the 56 generic entries of
csrc/sweep_variant.hpp -- the 15 pitched ones are tests/test_gpu_pitch.py's).  A row runs three sweeps, each compared with
the oracle and each held to the tile-visit kind it is there for (last_visit_counts):

  a. border geometry, LDS on   grid partly outside the field of view, 1 % NaN pixels in both images, lags of +-1 px in
                               both CRVALs x two CROTA values (helioprojective: through exactly 0.0, so that the zero lag's
                               border, parity and tap passes run with the row's pixel type and method): lds > interior,
                               the LDS window under the bounds rule;
  b. the same with use_lds 0   lds == 0 < visits: the global-memory gather;
  c. interior geometry         no NaN pixel, every tile (+) lag box inside the image: interior > 0 wherever the order is
                               compiled, all_finite > 0 exactly where the kernel has a clean path (kCleanPath,
                               kernels_sweep.hpp) and == 0 elsewhere.  A run-time-order kernel has no interior body at
                               all: interior == 0 is its design (`if constexpr (ORDER != ORDER_RT)`), asserted as such.
                               Carrington residus rows also run plain 'residus' here: finite for every lag.

After every sweep last_sweep_variant() is the entry the CPU test predicts (tests/test_sweep_variant_cases_cpu.py) with
the fields the row claims, and small_is_f32 is the row's pixel type.  A correlation sweep must also have re-evaluated NO
lag-point (refined_lag_points == 0): with a table entry swapped for its RESID neighbour's kernel, k_finalize found every
lag-point ill-conditioned, the re-evaluation about the lag-points' own means recomputed the whole map with other
kernels, and the map met the oracle all the same -- only this count told.

Tolerances are the project's own.  Correlation: NaN pattern equal, 1e-9 absolute on the Carrington frame, 1e-7 on the
helioprojective and plate-carree frames, the argmax rule of H.assert_corr_close.  Masked and plain residus: 1e-10 of
max|want| on the Carrington frame, 1e-5 of each entry on the others, the argmin rule of assert_masked
(tests/test_gpu_masked_scores.py); counts equal exactly.  Oracle maps are computed once per (frame, order, pixel type,
geometry) and shared by the rows of both methods.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import sweep_variant_cases as V
from tests.test_gpu_masked_scores import CARR_RTOL, HELIO_RTOL, assert_counts, assert_masked

pytestmark = pytest.mark.gpu


class OracleCache:
    """Oracle maps per (frame, order, pixel type, geometry), computed on first use and never modified."""

    def __init__(self):
        self._maps = {}

    def _get(self, fn, *key):
        k = (fn.__name__,) + key
        if k not in self._maps:
            out = fn(*key)
            for a in (out.values() if isinstance(out, dict) else [out]):
                a.setflags(write=False)
            self._maps[k] = out
        return self._maps[k]

    def correlation(self, row, geometry):
        return self._get(V.oracle_correlation, row.frame, row.order, row.f32_exact, geometry)

    def masked(self, row, geometry):
        return self._get(V.oracle_masked, row.frame, row.order, row.f32_exact, geometry)

    def plain_residus(self, row):
        return self._get(V.oracle_plain_residus, row.order, row.f32_exact)


@pytest.fixture(scope="module")
def oracle():
    return OracleCache()


def check_variant(h, row, what):
    v, want = h.last_sweep_variant(), V.claimed_variant(row)
    assert v["index"] == V.predicted()[V.row_id(row)], (what, v)
    assert tuple(v[k] for k in V.FIELDS[1:]) == want, (what, v, want)
    assert h.last_stats()["small_is_f32"] == int(row.f32_exact), what
    return want


def check_map(h, row, geometry, got, oracle, what):
    """The map and the counts of the sweep that just ran, against the oracles."""
    carr = row.frame == "carrington"
    m = oracle.masked(row, geometry)
    assert np.isfinite(m["masked"]).all() and m["poisoned"].sum() == 0, what  # (the oracle has a number for every lag)
    if row.method == "correlation":
        want = oracle.correlation(row, geometry)
        assert np.isfinite(want).all(), what
        print(f"\n[sweep variants] {what}: max|dcorr| = {np.nanmax(np.abs(got - want)):.3e}")
        H.assert_corr_close(got, want, 1e-9 if carr else 1e-7, what)
        assert_counts(h.last_counts(), m["count"], what)
        # the map is k_sweep's own: a lag-point whose sums look ill-conditioned is re-evaluated about its own means by
        # OTHER kernels (option "refine"), which repairs -- and so hides -- a k_sweep that accumulated the wrong sums
        assert h.last_visit_counts()["refined_lag_points"] == 0, what
    else:
        assert_masked(got, m["masked"], CARR_RTOL if carr else HELIO_RTOL, what, per_entry=not carr)
        assert_counts(h.last_counts(), m["finite_terms"], what)


@pytest.mark.parametrize("row", V.ROWS, ids=[V.row_id(r) for r in V.ROWS])
def test_instantiation_against_the_oracle(gpu_handle, oracle, row):
    h, name = gpu_handle, V.row_id(row)

    # a. border geometry, LDS on: the window under the bounds rule
    sweep = V.gpu_prepare(h, row, "border")
    got = sweep(row.method, use_lds=1)
    variant = check_variant(h, row, f"{name} (a)")
    vc = h.last_visit_counts()
    print(f"\n[sweep variants] {name} (a): {vc}")
    assert h.last_stats()["used_lds"] == 1 and vc["lds"] > vc["interior"] >= 0, vc
    check_map(h, row, "border", got, oracle, f"{name}, border, LDS")

    # b. the same with use_lds 0: the global-memory gather
    got = sweep(row.method, use_lds=0)
    check_variant(h, row, f"{name} (b)")
    vc = h.last_visit_counts()
    assert h.last_stats()["used_lds"] == 0 and vc["lds"] == 0 < vc["visits"], vc
    check_map(h, row, "border", got, oracle, f"{name}, border, global gather")

    # c. interior geometry
    sweep = V.gpu_prepare(h, row, "interior")
    got = sweep(row.method, use_lds=1)
    check_variant(h, row, f"{name} (c)")
    vc = h.last_visit_counts()
    print(f"\n[sweep variants] {name} (c): {vc}")
    assert vc["lds"] > 0, vc
    if variant[1] == V.ORDER_RT:
        # a run-time-order kernel compiles no interior body (kernels_sweep.hpp: `if constexpr (ORDER != ORDER_RT)`): its
        # LDS visits all keep the bounds rule -- by design, not for want of an interior tile
        assert vc["interior"] == 0 and vc["all_finite"] == 0, vc
    else:
        assert vc["interior"] > 0, vc
        assert (vc["all_finite"] > 0) == V.has_clean_path(variant) and vc["all_finite"] <= vc["interior"], vc
    check_map(h, row, "interior", got, oracle, f"{name}, interior")

    if row.frame == "carrington" and row.method == "residus_masked":
        # plain 'residus' on the full-overlap grid: a number for every lag, the same RESID instantiation
        got = sweep("residus", use_lds=1)
        check_variant(h, row, f"{name} (c, residus)")
        want = oracle.plain_residus(row)
        assert np.isfinite(want).all()
        assert_masked(got, want, CARR_RTOL, f"{name}, interior, plain residus")
        assert_counts(h.last_counts(), oracle.masked(row, "interior")["finite_terms"], f"{name}, plain residus")
