"""
CPU restatement (numpy only) of the destretch of a local shift field (`LocalShiftField.destretch`,
coreg_pixels_destretch), written out once from the rule of include/coreg_hip.h:

    D(Y, X) = S(Y - v(Y, X), X - u(Y, X))

with (u, v) the node values u[n_ty][n_tx], v[n_ty][n_tx] at the tile centres xs[n_tx], ys[n_ty] taken at the output
pixel's field coordinate (X', Y') = (X - col_offset, Y - row_offset), and S the order-1 sample of
tests/pxlshift_oracle.interpol2d (NaN outside the image, a NaN through any tap, the mirrored tap on the last pixel).
Every step is one float64 operation in the order the rule states, so the GPU's bits are these bits.
"""
import numpy as np

from . import pxlshift_oracle as O


def cell(c, p):
    """(i, f) of coordinates `p` on an axis of nodes `c`: i the largest index with c[i] <= p clamped to [0, n - 2],
    f = (p - c[i]) / (c[i + 1] - c[i]) clamped to [0, 1].  Not for an axis of one node."""
    c = np.asarray(c, dtype=np.float64)
    i = np.clip(np.searchsorted(c, p, side="right") - 1, 0, len(c) - 2)
    f = (p - c[i]) / (c[i + 1] - c[i])
    return i, np.minimum(np.maximum(f, 0.0), 1.0)


def displacement(shape, ys, xs, u, v, tile_shape, interpolation="bilinear", row_offset=0.0, col_offset=0.0):
    """[2][ny][nx]: (u, v) at every output pixel of an image of `shape`."""
    ny, nx = shape
    ys, xs = np.asarray(ys, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    Y, X = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    xp, yp = X - np.float64(col_offset), Y - np.float64(row_offset)
    if interpolation == "nearest":
        th, tw = tile_shape
        j = np.clip(np.floor(yp / np.float64(th)), 0, len(ys) - 1).astype(np.int64)
        i = np.clip(np.floor(xp / np.float64(tw)), 0, len(xs) - 1).astype(np.int64)
        return np.stack([u[j, i], v[j, i]])
    if interpolation != "bilinear":
        raise ValueError(interpolation)
    if len(xs) > 1:
        i, fx = cell(xs, xp)
    if len(ys) > 1:
        j, fy = cell(ys, yp)
    out = []
    for a in (u, v):
        def along_x(rows):  # an axis with one node is constant
            return a[rows, 0] if len(xs) == 1 else a[rows, i] * (1.0 - fx) + a[rows, i + 1] * fx
        if len(ys) == 1:
            out.append(along_x(np.zeros((ny, nx), dtype=np.int64)))
        else:
            out.append(along_x(j) * (1.0 - fy) + along_x(j + 1) * fy)
    return np.stack(out)


def destretch(data, ys, xs, u, v, tile_shape, interpolation="bilinear", row_offset=0.0, col_offset=0.0):
    """(planes of the shape and type of `data` [..., ny, nx], displacement [2][ny][nx])."""
    data = np.asarray(data)
    ny, nx = data.shape[-2:]
    d = displacement((ny, nx), ys, xs, u, v, tile_shape, interpolation, row_offset, col_offset)
    Y, X = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    x, y = X - d[0], Y - d[1]
    planes = data.reshape((-1, ny, nx))
    out = np.empty(planes.shape, dtype=data.dtype.newbyteorder("="))
    for k, plane in enumerate(planes):
        out[k] = O.interpol2d(plane, x, y, np.nan)  # (float64 sample, rounded once to the type of the data)
    return out.reshape(data.shape), d


def field_destretch(F, data, reference=None, interpolation="bilinear", fill="plane", row_offset=0, col_offset=0):
    """`destretch` with the nodes of a LocalShiftField: what `F.destretch(data, ...)` returns."""
    u, v = F.node_shifts(reference, fill)
    return destretch(data, F.tile_centres[:, 0, 1], F.tile_centres[0, :, 0], u, v, F.tile_shape, interpolation,
                     row_offset, col_offset)[0]
