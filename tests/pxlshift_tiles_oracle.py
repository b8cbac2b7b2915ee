"""
CPU restatement (numpy only) of the local shift field of the pixel-lag sweep, composed from the pieces of
tests/pxlshift_oracle.py and the definitions of tests/pxlshift_scores_oracle.py -- the same sub-resolved image,
displacement, rotation planes (rotated about the whole image's centre), slice origin and windows -- with every score and
count taken on the tile's rectangle of window and plane:

    tile (ty, tx) = rows [ty th, min(h, (ty + 1) th)) x columns [tx tw, min(w, (tx + 1) tw)) of the small-image plane
    corr          = the Pearson coefficient of pxlshift_oracle.correlate on the rectangle (its own means)
    masked        = np.std(((win - plane) / np.sqrt(win))[isfinite(win) & isfinite(plane)]) on the rectangle
"""
import numpy as np

from . import pxlshift_oracle as O

KEYS = ("corr", "count", "masked", "finite_terms", "poisoned")


def tile_slices(shape, tile_shape):
    """[n_ty][n_tx] of (row slice, column slice); the last tile of an axis may be ragged."""
    (h, w), (th, tw) = shape, tile_shape
    return [[(slice(r, min(h, r + th)), slice(c, min(w, c + tw))) for c in range(0, w, tw)] for r in range(0, h, th)]


def entry(win, plane):
    """The five figures of pxlshift_scores_oracle.scores for one window and plane (of any common shape)."""
    keep = np.isfinite(win) & np.isfinite(plane)
    with np.errstate(all="ignore"):
        d = ((win - plane) / np.sqrt(win))[keep]
        masked = np.std(d) if d.size else np.nan
    fin = np.isfinite(d)
    return (O.correlate(win, plane), np.count_nonzero(~(np.isnan(win) | np.isnan(plane))), masked, np.count_nonzero(fin),
            np.count_nonzero(~fin))


def scores(large, small, plan, tile_shape):
    """{"corr", "count", "masked", "finite_terms", "poisoned"}: float64 [n_ty][n_tx][n_dx][n_dy][n_rot] of an
    `AlignmentPixels.host_plan` dict on the images the object holds (`data_large`, `data_small`)."""
    large, small = np.asarray(large, dtype=np.float64), np.asarray(small, dtype=np.float64)
    if plan["shift_large"] is not None:
        large = O.shift_large(large, *plan["shift_large"])
    sub = O.sub_resolution(large, plan["ratio_res_1"], plan["ratio_res_2"])
    assert sub.shape == tuple(plan["sub_shape"])
    l = O.slice_origin(sub.shape, small.shape)
    assert tuple(l) == tuple(plan["slc_small_ref"])
    h, w = small.shape
    tiles = tile_slices((h, w), tile_shape)
    lag_dx, lag_dy, lag_drot = plan["lag_dx"], plan["lag_dy"], plan["lag_drot"]
    out = {k: np.full((len(tiles), len(tiles[0]), len(lag_dx), len(lag_dy), len(lag_drot)), np.nan) for k in KEYS}
    for k, drot in enumerate(lag_drot):
        plane = O.rotate(small, drot, plan["unit_rot"])
        for i, dx in enumerate(lag_dx):
            for j, dy in enumerate(lag_dy):
                r0, c0 = l[0] + int(dy), l[1] + int(dx)
                if r0 < 0 or c0 < 0 or r0 + h > sub.shape[0] or c0 + w > sub.shape[1]:
                    raise ValueError("too large shift : outside FSI")
                win = sub[r0:r0 + h, c0:c0 + w]
                for ty, row in enumerate(tiles):
                    for tx, (r, c) in enumerate(row):
                        for key, v in zip(KEYS, entry(win[r, c], plane[r, c])):
                            out[key][ty, tx, i, j, k] = v
    return out
