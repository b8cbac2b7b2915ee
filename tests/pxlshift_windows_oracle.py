"""
CPU restatement (numpy only) of the sliding, apodized windows of the local shift field,
composed from the pieces of tests/pxlshift_oracle.py, tests/pxlshift_tiles_oracle.py and tests/pxlshift_mi_oracle.py --
the same sub-resolved image, displacement, rotation planes (rotated about the whole image's centre), slice origin and
per-rectangle figures -- on the rectangles of a stepped grid:

    per axis of length h: one window when h <= th, else ceil((h - th) / sy) + 1
    window ty  = rows [ty sy, min(h, ty sy + th)); columns likewise

and, with weight tables (wy, wx), pixel (y, x) of the window at (r_lo, c_lo) weighted by w = wy[y - r_lo] * wx[x - c_lo]:

    keep = ~isnan(a) & ~isnan(b);  n = sum 1;  W = sum w;  am = sum w a / W;  bm = sum w b / W
    corr = float64(float32(sum w (a - am) (b - bm))) / sqrt(sum w (a - am)^2 * sum w (b - bm)^2)
    NaN when W = 0 or a weighted variance is 0; the count stays n

`scores` optionally takes prepared planes and a box in place of its own (the device's `A._rotated(k)`,
`A._large_box()`), as tests/pxlshift_mi_oracle.py does.
"""
import numpy as np

from . import pxlshift_mi_oracle as M
from . import pxlshift_oracle as O
from . import pxlshift_tiles_oracle as T

KEYS = T.KEYS + ("mi", "mi_count", "wcorr", "weight")


def axis_windows(n, size, step):
    """[(start, stop)] of the windows of `size` pixels, `step` apart, on an axis of `n` pixels."""
    count = 1 if n <= size else -(-(n - size) // step) + 1
    return [(k * step, min(n, k * step + size)) for k in range(count)]


def window_slices(shape, tile_shape, tile_step=None):
    """[n_ty][n_tx] of (row slice, column slice); tile_step None: the tile shape, the disjoint tiles."""
    step = tile_shape if tile_step is None else tile_step
    return [[(slice(*r), slice(*c)) for c in axis_windows(shape[1], tile_shape[1], step[1])]
            for r in axis_windows(shape[0], tile_shape[0], step[0])]


def gaussian_table(n, sigma):
    r = np.arange(n, dtype=np.float64)
    return np.exp(-0.5 * ((r - (n - 1) / 2) / sigma) ** 2)


def weights_of(wy, wx, shape):
    """The weights of a window of `shape` (a ragged one: the head of the tables), each one IEEE product."""
    return np.outer(np.asarray(wy, dtype=np.float64)[:shape[0]], np.asarray(wx, dtype=np.float64)[:shape[1]])


def weighted(win, plane, w):
    """(corr, n, W) of a window of the large image, the plane under it and the weights, all of one shape."""
    a, b, w = plane.ravel(), win.ravel(), np.asarray(w, dtype=np.float64).ravel()
    keep = ~np.isnan(a) & ~np.isnan(b)
    a, b, w = a[keep], b[keep], w[keep]
    n, W = int(keep.sum()), float(w.sum())
    if W == 0.0:
        return np.nan, n, W
    with np.errstate(all="ignore"):
        da, db = a - (w * a).sum() / W, b - (w * b).sum() / W
        num, va, vb = np.float32((w * da * db).sum()), (w * da * da).sum(), (w * db * db).sum()
        if va == 0.0 or vb == 0.0:
            return np.nan, n, W
        return float(np.float64(num) / np.sqrt(va * vb)), n, W


def scores(large, small, plan, tile_shape, tile_step=None, window=None, planes=None, box=None, mi=False):
    """{key: float64 [n_ty][n_tx][n_dx][n_dy][n_rot]} of an `AlignmentPixels.host_plan` dict on the images the object holds:
    the five keys of pxlshift_tiles_oracle.scores; with mi (a plan of method "mutual_information"), "mi" and "mi_count";
    with window = (wy, wx), "wcorr" and "weight" (W).  planes: [n_rot] arrays [h][w] in place of the oracle's rotated
    planes; box: the sub-resolved image from (l0 + min dy, l1 + min dx) on in place of the oracle's."""
    small = np.asarray(small, dtype=np.float64)
    h, w = small.shape
    l = list(plan["slc_small_ref"])
    lag_dx, lag_dy, lag_drot = plan["lag_dx"], plan["lag_dy"], plan["lag_drot"]
    if box is None:
        large = np.asarray(large, dtype=np.float64)
        if plan["shift_large"] is not None:
            large = O.shift_large(large, *plan["shift_large"])
        sub = O.sub_resolution(large, plan["ratio_res_1"], plan["ratio_res_2"])
        assert sub.shape == tuple(plan["sub_shape"]) and O.slice_origin(sub.shape, small.shape) == l
        r_org, c_org = 0, 0
    else:
        sub = np.asarray(box, dtype=np.float64)
        r_org, c_org = l[0] + int(lag_dy.min()), l[1] + int(lag_dx.min())
        assert sub.shape == (h + int(lag_dy.max() - lag_dy.min()), w + int(lag_dx.max() - lag_dx.min()))
    tiles = window_slices((h, w), tile_shape, tile_step)
    keys = T.KEYS + (("mi", "mi_count") if mi else ()) + (("wcorr", "weight") if window is not None else ())
    out = {k: np.full((len(tiles), len(tiles[0]), len(lag_dx), len(lag_dy), len(lag_drot)), np.nan) for k in keys}
    for k, drot in enumerate(lag_drot):
        plane = O.rotate(small, drot, plan["unit_rot"]) if planes is None else np.asarray(planes[k], dtype=np.float64)
        for i, dx in enumerate(lag_dx):
            for j, dy in enumerate(lag_dy):
                r0, c0 = l[0] + int(dy) - r_org, l[1] + int(dx) - c_org
                if r0 < 0 or c0 < 0 or r0 + h > sub.shape[0] or c0 + w > sub.shape[1]:
                    raise ValueError("too large shift : outside FSI")
                win = sub[r0:r0 + h, c0:c0 + w]
                for ty, row in enumerate(tiles):
                    for tx, (r, c) in enumerate(row):
                        at = (ty, tx, i, j, k)
                        for key, v in zip(T.KEYS, T.entry(win[r, c], plane[r, c])):
                            out[key][at] = v
                        if mi:
                            out["mi"][at], out["mi_count"][at] = M.entry(plane[r, c], win[r, c], *plan["bins"])
                        if window is not None:
                            wgt = weights_of(window[0], window[1], plane[r, c].shape)
                            out["wcorr"][at], n, out["weight"][at] = weighted(win[r, c], plane[r, c], wgt)
                            assert n == out["count"][at]
    return out
