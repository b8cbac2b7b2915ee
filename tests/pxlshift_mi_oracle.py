"""
CPU restatement (numpy only) of the mutual-information score of the pixel-lag sweep, composed
from the pieces of tests/pxlshift_oracle.py -- the same sub-resolved image, displacement, rotation planes, slice origin
and windows -- with, per lag (and per tile),

    a, b  = the (rotated) small-image plane and the window of the sub-resolved large image under it
    keep  = ~isnan(a) & ~isnan(b)                                  (an infinite pixel is kept: it falls into an end bin)
    bin   = np.searchsorted(edges, v, side="right")                (the number of edges <= v)
    n_ij  = np.add.at over (bin(a), bin(b)) of the kept pairs;  n, r_i, c_j its total, row sums and column sums
    MI    = sum over n_ij > 0 of (n_ij / n) log((n_ij n) / (r_i c_j))    float64, nats;  NaN for n = 0

`scores` optionally takes prepared planes and a box in place of its own (the device's `A._rotated(k)`,
`A._large_box()`): the bins are then those of identical pixels.
"""
import numpy as np

from . import pxlshift_oracle as O
from .pxlshift_tiles_oracle import tile_slices


def histogram(a, b, edges_small, edges_large):
    """The joint histogram [len(edges_small) + 1][len(edges_large) + 1] (int64) of two arrays of one shape."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    keep = ~np.isnan(a) & ~np.isnan(b)
    ia = np.searchsorted(np.asarray(edges_small, dtype=np.float64), a[keep], side="right")
    ib = np.searchsorted(np.asarray(edges_large, dtype=np.float64), b[keep], side="right")
    hist = np.zeros((len(edges_small) + 1, len(edges_large) + 1), dtype=np.int64)
    np.add.at(hist, (ia, ib), 1)
    return hist


def mi_of_histogram(hist):
    """The score of a joint histogram of integer counts: nats, NaN when it is empty."""
    hist = np.asarray(hist)
    n = int(hist.sum())
    if n == 0:
        return np.nan
    r, c = hist.sum(axis=1, keepdims=True).astype(np.float64), hist.sum(axis=0, keepdims=True).astype(np.float64)
    nij = hist.astype(np.float64)
    pos = hist > 0
    ratio = (nij * float(n))[pos] / (r * c)[pos]
    return float(np.sum((nij[pos] / float(n)) * np.log(ratio)))


def entry(a, b, edges_small, edges_large):
    """(MI, n) of a plane and the window under it."""
    hist = histogram(a, b, edges_small, edges_large)
    return mi_of_histogram(hist), int(hist.sum())


def scores(large, small, plan, planes=None, box=None, tile_shape=None):
    """{"mi", "count"}: float64 cubes [n_dx][n_dy][n_rot] -- with `tile_shape`, [n_ty][n_tx][n_dx][n_dy][n_rot] -- of an
    `AlignmentPixels.host_plan(method="mutual_information")` dict on the images the object holds.  planes: [n_rot] arrays
    [h][w] in place of the oracle's rotated planes; box: the sub-resolved image from (l0 + min dy, l1 + min dx) on in
    place of the oracle's."""
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
    es, el = plan["bins"]
    tiles = [[(slice(0, h), slice(0, w))]] if tile_shape is None else tile_slices((h, w), tile_shape)
    shape = (len(tiles), len(tiles[0]), len(lag_dx), len(lag_dy), len(lag_drot))
    out = {"mi": np.full(shape, np.nan), "count": np.full(shape, np.nan)}
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
                        out["mi"][ty, tx, i, j, k], out["count"][ty, tx, i, j, k] = entry(plane[r, c], win[r, c], es, el)
    if tile_shape is None:
        out = {key: v[0, 0] for key, v in out.items()}
    return out


def scene(seed=1, shape=(24, 20), lag=(-2, 3), pad=8):
    """A scene where the relation between the two intensities is not monotonic: a smooth log-normal large image, and a
    small image cut from it at the injected lag (dx, dy) and passed through |log(x / median)| with noise and a NaN block.
    Returns (large, small, keyword arguments of the sweep)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    H, W = h + 2 * pad, w + 2 * pad
    raw = rng.normal(0.0, 1.0, (H, W))
    for _ in range(3):  # three 3 x 3 box means, edges by wrap-around: structure a few pixels wide
        raw = sum(np.roll(np.roll(raw, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    large = np.exp(2.0 * raw / raw.std())
    l = O.slice_origin((H, W), (h, w))
    dx, dy = lag
    cut = large[l[0] + dy:l[0] + dy + h, l[1] + dx:l[1] + dx + w]
    small = np.abs(np.log(cut / np.median(cut))) + rng.normal(0.0, 0.05, (h, w))
    small[3:6, 4:8] = np.nan
    kw = dict(lag_dx=np.arange(-4, 5), lag_dy=np.arange(-4, 5), lag_drot=np.array([0.0]))
    return large, small, kw
