"""
CPU restatement (numpy only) of the reference's pixel-lag alignment, the readable pin of
tests/golden/pxlshift_golden.*: `pxlshift/alignment_pixels.py`, `pxlshift/c_correlate.py:41-63`,
`utils/matrix_transform.py:78-106` and scipy.ndimage.map_coordinates(order=1, mode='constant', prefilter=False).

The order-1 sample is written out in scipy's own order of operations -- taps row by row, each (pixel * wy) * wx, summed
from 0 -- so that unrotated planes equal the reference to the bit whatever scipy is installed.
"""
import numpy as np


def interpol2d(image, x, y, fill):
    """rectify.interpol2d(image, x, y, order=1, fill=fill) (utils/rectify.py:22-56)."""
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inb = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    xs, ys = np.where(inb, x, 0.0), np.where(inb, y, 0.0)
    fx, fy = np.floor(xs), np.floor(ys)
    tx, ty = xs - fx, ys - fy
    wx, wy = (1.0 - tx, tx), (1.0 - ty, ty)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    # one past the last pixel (coordinate exactly n - 1, weight 0): the mirrored pixel n - 2
    xi = (x0, np.where(x0 + 1 < W, x0 + 1, max(W - 2, 0)))
    yi = (y0, np.where(y0 + 1 < H, y0 + 1, max(H - 2, 0)))
    t = np.zeros(x.shape, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for a in range(2):
            for b in range(2):
                t = t + (image[yi[a], xi[b]] * wy[a]) * wx[b]
    return np.where(inb, t, float(fill))


def fill_to_nan(a, fill):
    a = np.array(a, dtype=np.float64)
    a[a == fill] = np.nan
    return a


def sub_resolution(large, ratio1, ratio2):
    """alignment_pixels.py:126-143."""
    x, y = np.meshgrid(np.arange(0, large.shape[1], ratio1), np.arange(0, large.shape[0], ratio2))
    return fill_to_nan(interpol2d(large, x, y, -32768), -32768)


def slice_origin(sub_shape, small_shape):
    """alignment_pixels.py:145-148."""
    return [int((sub_shape[n] - small_shape[n] - 1) / 2) for n in range(2)]


def rotate(small, drot, unit_rot="degree"):
    """alignment_pixels.py:72-81 with matrix_transform.polar_transform; drot == 0: the image itself."""
    if drot == 0:
        return np.array(small, dtype=np.float64)
    if unit_rot == "degree":
        theta = np.radians(drot)
    elif unit_rot == "radian":
        theta = drot
    else:
        raise ValueError(unit_rot)
    xx, yy = np.meshgrid(np.arange(small.shape[1]), np.arange(small.shape[0]))
    xc, yc = round(small.shape[1] / 2), round(small.shape[0] / 2)
    nr = np.sqrt(np.power(xx - xc, 2) + np.power(yy - yc, 2))
    nt = np.arctan2(yy - yc, xx - xc) + theta
    nx, ny = nr * np.cos(nt) + xc, nr * np.sin(nt) + yc
    return fill_to_nan(interpol2d(small, nx, ny, -32762), -32762)


def shift_large(large, dx, dy):
    """alignment_pixels.py:86-107 given the displacement."""
    xx, yy = np.meshgrid(np.arange(large.shape[1]), np.arange(large.shape[0]))
    out = fill_to_nan(interpol2d(large, xx, yy, -32762), -32762)
    return fill_to_nan(interpol2d(out, xx + dx, yy + dy, -32762), -32762)


def correlate(window, plane):
    """alignment_pixels.py:49-55 + c_correlate.py:41-63 at lag 0: float32 numerator, float64 quotient."""
    keep = ~(np.isnan(window.ravel()) | np.isnan(plane.ravel()))
    s1, s2 = plane.ravel()[keep], window.ravel()[keep]
    with np.errstate(all="ignore"):
        c1, c2 = s1 - s1.mean(), s2 - s2.mean()
        num = np.float32((c1 * c2).sum())
        return float(np.float64(num) / np.sqrt((c1 ** 2).sum() * (c2 ** 2).sum()))


def sweep(sub, small, lag_dx, lag_dy, lag_drot, unit_rot="degree"):
    """alignment_pixels.py:57-84 on the sub-resolved image."""
    h, w = small.shape
    l = slice_origin(sub.shape, small.shape)
    corr = np.zeros((len(lag_dx), len(lag_dy), len(lag_drot)), dtype=np.float64)
    for k, drot in enumerate(lag_drot):
        plane = rotate(small, drot, unit_rot)
        for i, dx in enumerate(lag_dx):
            for j, dy in enumerate(lag_dy):
                r0, c0 = l[0] + int(dy), l[1] + int(dx)
                if r0 < 0 or c0 < 0 or r0 + h > sub.shape[0] or c0 + w > sub.shape[1]:
                    raise ValueError("too large shift : outside FSI")
                corr[i, j, k] = correlate(sub[r0:r0 + h, c0:c0 + w], plane)
    return corr
