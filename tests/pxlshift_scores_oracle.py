"""
CPU restatement (numpy only) of the scores and sample counts of the pixel-lag sweep, composed from the pieces of
tests/pxlshift_oracle.py -- the same sub-resolved image, displacement, rotation planes, slice origin and Pearson
coefficient, walked over the same windows -- plus the masked residus of this project:

    win   = window of the sub-resolved large image (the reference image), plane = the (rotated) small image
    keep  = isfinite(win) & isfinite(plane)
    score = np.std(((win - plane) / np.sqrt(win))[keep])          ddof 0; NaN for an empty selection

A kept term that is not finite (win <= 0) is "poisoned": numpy's std of a selection holding one is NaN.
"""
import numpy as np

from . import pxlshift_oracle as O


def scores(large, small, plan):
    """{"corr", "count", "masked", "finite_terms", "poisoned"}: float64 cubes [n_dx][n_dy][n_rot] of a
    `AlignmentPixels.host_plan` dict on the images the object holds (`data_large`, `data_small`)."""
    large, small = np.asarray(large, dtype=np.float64), np.asarray(small, dtype=np.float64)
    if plan["shift_large"] is not None:
        large = O.shift_large(large, *plan["shift_large"])
    sub = O.sub_resolution(large, plan["ratio_res_1"], plan["ratio_res_2"])
    assert sub.shape == tuple(plan["sub_shape"])
    l = O.slice_origin(sub.shape, small.shape)
    assert tuple(l) == tuple(plan["slc_small_ref"])
    h, w = small.shape
    lag_dx, lag_dy, lag_drot = plan["lag_dx"], plan["lag_dy"], plan["lag_drot"]
    out = {k: np.full((len(lag_dx), len(lag_dy), len(lag_drot)), np.nan)
           for k in ("corr", "count", "masked", "finite_terms", "poisoned")}
    for k, drot in enumerate(lag_drot):
        plane = O.rotate(small, drot, plan["unit_rot"])
        for i, dx in enumerate(lag_dx):
            for j, dy in enumerate(lag_dy):
                r0, c0 = l[0] + int(dy), l[1] + int(dx)
                if r0 < 0 or c0 < 0 or r0 + h > sub.shape[0] or c0 + w > sub.shape[1]:
                    raise ValueError("too large shift : outside FSI")
                win = sub[r0:r0 + h, c0:c0 + w]
                out["corr"][i, j, k] = O.correlate(win, plane)
                out["count"][i, j, k] = np.count_nonzero(~(np.isnan(win) | np.isnan(plane)))
                keep = np.isfinite(win) & np.isfinite(plane)
                with np.errstate(all="ignore"):
                    d = ((win - plane) / np.sqrt(win))[keep]
                    out["masked"][i, j, k] = np.std(d) if d.size else np.nan
                fin = np.isfinite(d)
                out["finite_terms"][i, j, k] = np.count_nonzero(fin)
                out["poisoned"][i, j, k] = np.count_nonzero(~fin)
    return out
