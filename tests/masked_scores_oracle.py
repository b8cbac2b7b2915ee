"""numpy oracle of the masked residus and of the per-lag sample counts, composed from the CPU oracle's own building blocks
(oracle/coreg_oracle.py: set_initial_header_values, lag_table, prepare_reference, shift_header, carrington_transform_fa,
interpolate_on_large_data_grid; oracle/context_oracle.py: context_step(..., samples=True)).  For every lag-point:

  A = reference image on the target grid, B = resampled image to align, mask = isfinite(A) & isfinite(B)
  count    = mask.sum()
  masked   = np.std(((A - B) / sqrt(A))[mask])      ddof 0; NaN, as numpy returns it, for an empty mask or a term
                                                    that is not finite (A <= 0)
  poisoned = number of masked terms that are not finite

The arithmetic is the oracle's `residus` (alignment.py:544-547) in the arrays' own dtypes, so that the masked score equals
the unmasked one wherever every grid point overlaps."""
import warnings

import numpy as np

from oracle import context_oracle as CO
from oracle import coreg_oracle as O


def masked_terms(A, B):
    """(count of co-finite points, np.std of their terms, number of terms that are not finite)."""
    a, b = np.asarray(A).ravel(), np.asarray(B).ravel()
    mask = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = ((a - b) / np.sqrt(a))[mask]
        score = float(np.std(d)) if d.size else np.nan
    return int(mask.sum()), score, int((~np.isfinite(d)).sum())


def pearson_count(A, B):
    """Samples of the Pearson sums (alignment.py:525-531)."""
    return int((np.isfinite(np.asarray(A).ravel()) & np.isfinite(np.asarray(B).ravel())).sum())


def sweep(st, frame, parallelism=True, use_ang2pipi=True):
    """The whole sweep of `st` (tests/helpers.oracle_state): dict of 6-D arrays [crval1, crval2, cdelt1, cdelt2, crota,
    solar_r] -- "masked" (the masked residus), "count" (co-finite points), "finite_terms" (count minus the poisoned
    terms: what the library reports for the residus methods), "poisoned".  A lag-point without a map: NaN everywhere."""
    O.set_initial_header_values(st, use_ang2pipi)
    table, shp = O.lag_table(st)
    nsr = len(st.lag_solar_r)
    out = {k: np.full((table.shape[0], nsr), np.nan) for k in ("masked", "count", "finite_terms", "poisoned")}
    for kk, d_solar_r in enumerate(st.lag_solar_r):
        A = O.prepare_reference(st, frame, d_solar_r, parallelism)
        for i, lg in enumerate(table):
            hdr = dict(st.hdr_small)
            O.shift_header(st, hdr, *lg)
            if frame == "carrington":
                B = O.carrington_transform_fa(st.data_small, hdr, d_solar_r, st.shape, st.lonlims, st.latlims, st.order)
            else:
                try:
                    B = O.interpolate_on_large_data_grid(st, st.data_small, hdr)
                except O.InvalidTransformError:
                    continue
            n, score, bad = masked_terms(A, B)
            out["masked"][i, kk], out["count"][i, kk] = score, n
            out["finite_terms"][i, kk], out["poisoned"][i, kk] = n - bad, bad
    return {k: v.reshape(shp + (nsr,)) for k, v in out.items()}


def context_sweep(case):
    """The iterative-context sweep of a tests/context_cases case: the same dict of arrays, shaped as the five lag axes.  A
    masked term needs both samples finite and the SPICE sample inside the thresholds."""
    axes, table = CO.lag_table(case["lags"])
    out = {k: np.full(table.shape[0], np.nan) for k in ("masked", "count", "finite_terms", "poisoned")}
    for i, lag in enumerate(table):
        _, a, b = CO.context_step(case["frames"], case["frame_headers"], case["col_frame"], case["spice"],
                                  case["target4"], case["hdr_small"], lag, order=case["order"], method="residus",
                                  semantics=case["semantics"], vmin=case["vmin"], vmax=case["vmax"], samples=True)
        if a is None:
            continue
        bf = b.astype(np.float32)
        with np.errstate(invalid="ignore"):
            if case["vmin"] is not None:
                b = np.where(bf > np.float32(case["vmin"]), b, np.nan)
            if case["vmax"] is not None:
                b = np.where(bf < np.float32(case["vmax"]), b, np.nan)
        n, score, bad = masked_terms(a, b)
        out["masked"][i], out["count"][i], out["finite_terms"][i], out["poisoned"][i] = score, n, n - bad, bad
    return {k: v.reshape([len(x) for x in axes]) for k, v in out.items()}
