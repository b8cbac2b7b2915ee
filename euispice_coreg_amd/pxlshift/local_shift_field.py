"""
`LocalShiftField` -- what `AlignmentPixels.find_local_shifts` returns: the small image cut into tiles, and per tile the
cube of the integer pixel-lag sweep on the tile's own rectangle (`corr[n_ty, n_tx, n_dx, n_dy, n_rot]`), the sample
count behind every entry (`n_samples`, taken before `min_overlap`), the best entry (maximum of a correlation or of
`mutual_information`, minimum of `residus_masked`) and its sub-lag position -- the one Gaussian fit
`PixelAlignmentResults` runs (`hdrshift.alignment_results.gaussian_sub_lag`), on the tile's (dx, dy) plane at its best rotation, the best entry
itself where the fit cannot run or fails.

A tile is `valid` when its largest count reaches `min_fill` times its pixel count and a finite entry is left after
`min_overlap` (a count, or a fraction of that tile's own largest count: `hdrshift.alignment.apply_min_overlap` per
tile).  An invalid tile raises nothing: its shifts, score and rotation are NaN and its `best_index` is -1.  Only a field
without any valid tile raises ValueError.

With `tile_step` = (sy, sx) the tiles are windows whose origins lie a step apart, the tile shape or less
(`alignment_pixels.tile_grid`): they overlap, and the field has a node per window.  With weight tables (`window`, the
apodization of `find_local_shifts`) `weight_sums` holds the sum of the kept pixels' weights behind every entry; the count
of an entry stays the kept pixels, and a tile is then valid when its largest weight sum reaches `min_fill` times the
sum of the weights over its rectangle -- kept pixels in the corners of a bell do not make it valid.  A ragged window's
weights are the head of the tables; its centre in `tile_centres` stays the centre of the clipped rectangle.

From the valid tiles: `median_shift` and `scatter` (1.4826 x the median absolute deviation) of dx and dy -- an empirical
error bar on a global shift -- and `drift()`, the least-squares planes of dx and dy over the tile centres: the drift
across a raster.

There is no FITS card for a tile-dependent correction: the field is applied to the pixels instead.  `node_shifts` gives
the field as node values at the tile centres (host only); `destretch` resamples an image, or a stack of planes, by it
(include/coreg_hip.h: coreg_pixels_destretch, the rule is stated there), so that the result lies on its own grid at one
rigid shift, the `reference`; `AlignmentSpicePixel.write_destretched_fits` writes the planes of SPICE windows so corrected.
"""
from __future__ import annotations

import os

import numpy as np

from ..hdrshift.alignment import apply_min_overlap, min_overlap_floor
from ..hdrshift.alignment_results import gaussian_sub_lag
from .alignment_pixels import check_tile_step, tile_grid, window_slices
from .pixel_alignment_results import _BEST


_FILLS = ("plane", "median", "zero")
_INTERPOLATIONS = ("bilinear", "nearest")  # (the library's codes: 0, 1)
MAX_ELEMENTS = 2 ** 31 - 1  # of one coreg_pixels_destretch call


class LocalShiftField:

    def __init__(self, corr, n_samples, lag_dx, lag_dy, lag_drot, tile_shape, image_shape, unit_rot="degree",
                 method="correlation", min_overlap=None, min_fill=0.5, sub_lag=True, fit=None, tile_step=None,
                 weight_sums=None, window=None):
        if method not in _BEST:
            raise NotImplementedError
        fit = fit or os.environ.get("COREG_GAUSSIAN_FIT", "native")
        if fit not in ("native", "scipy"):
            raise ValueError("fit must be 'native' or 'scipy'")
        if min_overlap is not None:
            min_overlap_floor(min_overlap)  # (a value that is neither a count nor a fraction raises here, not per tile)
        if not 0.0 <= min_fill <= 1.0:
            raise ValueError("min_fill must lie in [0, 1]")
        self.fit, self.method, self.best, self.unit_rot = fit, method, _BEST[method], unit_rot
        self.min_overlap, self.min_fill, self.sub_lag = min_overlap, float(min_fill), bool(sub_lag)
        self.lag_dx, self.lag_dy, self.lag_drot = (np.atleast_1d(np.asarray(v)) for v in (lag_dx, lag_dy, lag_drot))
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.tile_shape, grid = tile_grid(self.image_shape, tile_shape, tile_step)
        self.tile_step = check_tile_step(self.tile_shape, tile_step)
        corr, n_samples = np.asarray(corr, dtype=np.float64), np.asarray(n_samples, dtype=np.float64)
        if corr.shape != grid + (len(self.lag_dx), len(self.lag_dy), len(self.lag_drot)) or n_samples.shape != corr.shape:
            raise ValueError("corr and n_samples must be shaped [n_ty, n_tx, len(lag_dx), len(lag_dy), len(lag_drot)]")
        self.n_samples = n_samples
        if (weight_sums is None) != (window is None):
            raise ValueError("weight_sums and window (the weight tables) come together")
        self.weight_sums = self.window = None
        if window is not None:
            if method != "correlation":
                raise ValueError("apodization belongs to method='correlation'")
            self.weight_sums = np.asarray(weight_sums, dtype=np.float64)
            self.window = tuple(np.asarray(t, dtype=np.float64) for t in window)
            if self.weight_sums.shape != corr.shape or tuple(t.shape for t in self.window) != tuple(
                    (n,) for n in self.tile_shape):
                raise ValueError("weight_sums must be shaped like corr, the weight tables like the tile shape")
        self.corr = np.full(corr.shape, np.nan)  # (after min_overlap; an emptied tile is all NaN)
        self.tile_slices = window_slices(self.image_shape, self.tile_shape, self.tile_step)
        # (x, y) of every tile's centre in small-image pixels
        self.tile_centres = np.array([[((c.start + c.stop - 1) / 2, (r.start + r.stop - 1) / 2) for r, c in row]
                                      for row in self.tile_slices], dtype=np.float64)
        self.valid = np.zeros(grid, dtype=bool)
        self.fitted = np.zeros(grid, dtype=bool)
        self.best_index = np.full(grid + (3,), -1, dtype=np.int64)
        self.best_score, self.shift_dx, self.shift_dy, self.drot = (np.full(grid, np.nan) for _ in range(4))
        for ty in range(grid[0]):
            for tx in range(grid[1]):
                self._tile(ty, tx, corr[ty, tx])
        if not self.valid.any():
            raise ValueError("no valid tile: none holds min_fill of its pixels at any lag with a finite entry left")

    def _tile(self, ty, tx, cube):
        counts = self.n_samples[ty, tx]
        try:
            cube = apply_min_overlap(cube, counts, self.min_overlap)
        except ValueError:  # (the floor leaves no entry of this tile)
            return
        self.corr[ty, tx] = cube
        r, c = self.tile_slices[ty][tx]
        if self.window is None:
            filled = np.nanmax(counts) >= self.min_fill * ((r.stop - r.start) * (c.stop - c.start))
        else:  # the weights the window holds against those of its rectangle (a ragged one: the head of the tables)
            full = np.outer(self.window[0][:r.stop - r.start], self.window[1][:c.stop - c.start]).sum()
            filled = np.nanmax(self.weight_sums[ty, tx]) >= self.min_fill * full
        if not (np.isfinite(cube).any() and filled):
            return
        mi = np.unravel_index((np.nanargmin if self.best == "min" else np.nanargmax)(cube), cube.shape)
        pos = None
        if self.sub_lag:
            pos, _ = gaussian_sub_lag(cube[:, :, mi[2]], (mi[0], mi[1]), self.best, self.fit)
        x, y = (mi[0], mi[1]) if pos is None else (pos[0], pos[1])
        self.valid[ty, tx] = True
        self.fitted[ty, tx] = pos is not None
        self.best_index[ty, tx] = mi
        self.best_score[ty, tx] = cube[mi]
        self.shift_dx[ty, tx] = np.interp(x, np.arange(len(self.lag_dx)), self.lag_dx)
        self.shift_dy[ty, tx] = np.interp(y, np.arange(len(self.lag_dy)), self.lag_dy)
        self.drot[ty, tx] = self.lag_drot[mi[2]]

    @property
    def median_shift(self):
        """(dx, dy): the medians over the valid tiles."""
        return float(np.median(self.shift_dx[self.valid])), float(np.median(self.shift_dy[self.valid]))

    @property
    def scatter(self):
        """(dx, dy): 1.4826 x the median absolute deviation over the valid tiles (sigma of a normal scatter)."""
        return tuple(float(1.4826 * np.median(np.abs(v[self.valid] - np.median(v[self.valid]))))
                     for v in (self.shift_dx, self.shift_dy))

    def drift(self):
        """[[a0, a1, a2], [b0, b1, b2]]: the least-squares planes dx = a0 + a1 xc + a2 yc, dy = b0 + b1 xc + b2 yc over
        the centres (xc, yc) of the valid tiles.  ValueError with fewer than three valid tiles or collinear centres."""
        xy = self.tile_centres[self.valid]
        if len(xy) < 3:
            raise ValueError("drift needs at least three valid tiles")
        M = np.column_stack([np.ones(len(xy)), xy[:, 0], xy[:, 1]])
        if np.linalg.matrix_rank(M) < 3:
            raise ValueError("drift needs tile centres that are not collinear")
        sol = np.linalg.lstsq(M, np.column_stack([self.shift_dx[self.valid], self.shift_dy[self.valid]]), rcond=None)[0]
        return sol.T.copy()

    # ------------------------------------------------------------------------------------------------- destretch
    def _reference(self, reference):
        if reference is None:
            return self.median_shift
        try:
            rx, ry = (float(r) for r in reference)
        except (TypeError, ValueError):
            raise ValueError("reference must be None or a pair (rx, ry) of pixels") from None
        if not (np.isfinite(rx) and np.isfinite(ry)):
            raise ValueError("reference must be finite")
        return rx, ry

    def node_shifts(self, reference=None, fill="plane"):
        """(u, v), each [n_ty, n_tx]: the shifts of the tiles about the rigid shift `reference` = (rx, ry), default
        `median_shift` -- u = dx - rx, v = dy - ry -- the node values of the field at `tile_centres`.  An invalid tile
        is filled: "plane" (the `drift()` planes at the tile's centre; "median" where `drift()` raises), "median"
        (`median_shift`) or "zero" (the reference itself: no displacement).  ValueError for a node that is still not
        finite.  Host only."""
        if fill not in _FILLS:
            raise ValueError(f"fill must be one of {_FILLS}")
        rx, ry = self._reference(reference)
        dx, dy = self.shift_dx.copy(), self.shift_dy.copy()
        bad = ~self.valid
        if bad.any():
            plane = None
            if fill == "plane":
                try:
                    plane = self.drift()
                except ValueError:
                    fill = "median"
            if plane is not None:
                xc, yc = self.tile_centres[..., 0], self.tile_centres[..., 1]
                dx[bad] = (plane[0, 0] + plane[0, 1] * xc + plane[0, 2] * yc)[bad]
                dy[bad] = (plane[1, 0] + plane[1, 1] * xc + plane[1, 2] * yc)[bad]
            elif fill == "median":
                dx[bad], dy[bad] = self.median_shift
            else:
                dx[bad], dy[bad] = rx, ry
        u, v = dx - rx, dy - ry
        if not (np.isfinite(u).all() and np.isfinite(v).all()):
            raise ValueError("a node of the field is not finite")
        return u, v

    def destretch(self, data, reference=None, interpolation="bilinear", fill="plane", row_offset=0, col_offset=0,
                  return_displacement=False, device=None):
        """`data` resampled by the field so that it lies on its own grid at the rigid shift `reference` (default
        `median_shift`): D(Y, X) = S(Y - v(Y, X), X - u(Y, X)), order 1, NaN where the sample leaves the image, with
        (u, v) the `node_shifts(reference, fill)` interpolated to the output pixel -- "bilinear" between the tile centres
        and constant beyond the outer ones, or "nearest", the value of the pixel's tile.  The rule is written out in
        include/coreg_hip.h (coreg_pixels_destretch); the best rotations of the tiles are not applied.

        data: [h, w] or any stack [..., ny, nx] of float32 / float64, every plane resampled alike (a big-endian view of a
        FITS data unit is converted on the host; the result is in native byte order).  Pixel (Y, X) of a plane has field
        coordinate (Y - row_offset, X - col_offset): for planes taller or wider than the image the field was measured on.
        Returns an array of the shape and type of `data`; with return_displacement, also the displacement [2, ny, nx]
        = (u, v) of every output pixel."""
        if interpolation not in _INTERPOLATIONS:
            raise ValueError(f"interpolation must be one of {_INTERPOLATIONS}")
        if interpolation == "nearest" and self.tile_step != self.tile_shape:
            raise ValueError("interpolation='nearest' is the value of the pixel's tile: overlapping windows "
                             "(tile_step != tile_shape) have none, use 'bilinear'")
        u, v = self.node_shifts(reference, fill)
        a = np.asarray(data)
        if a.dtype.kind != "f" or a.dtype.itemsize not in (4, 8):
            raise TypeError("destretch takes float32 or float64 data")
        if a.ndim < 2 or a.size == 0:
            raise ValueError("destretch takes an image [h, w] or a stack [..., ny, nx]")
        row_offset, col_offset = float(row_offset), float(col_offset)
        if not (np.isfinite(row_offset) and np.isfinite(col_offset)):
            raise ValueError("row_offset and col_offset must be finite")
        native = a.dtype.newbyteorder("=")
        ny, nx = a.shape[-2:]
        planes = a.reshape((-1, ny, nx))
        from .. import _lib
        hnd = _lib.shared_handle(-1 if device is None else device)
        xs, ys = self.tile_centres[0, :, 0], self.tile_centres[:, 0, 1]
        out = np.empty(planes.shape, dtype=native)
        disp = None
        step = max(1, MAX_ELEMENTS // (ny * nx))  # planes per call: the library takes 2^31 - 1 elements at most
        for p0 in range(0, len(planes), step):
            part = np.ascontiguousarray(planes[p0:p0 + step], dtype=native)
            got = hnd.pixels_destretch(part, ys, xs, u, v, self.tile_shape, _INTERPOLATIONS.index(interpolation),
                                       row_offset, col_offset, return_displacement=return_displacement and p0 == 0)
            if return_displacement and p0 == 0:
                got, disp = got
            out[p0:p0 + step] = got
        out = out.reshape(a.shape)
        return (out, disp) if return_displacement else out

    def __str__(self):
        (mx, my), (sx, sy) = self.median_shift, self.scatter
        return (f"\n Local shifts : {int(self.valid.sum())} valid of {self.valid.size} tiles of {self.tile_shape[0]} x "
                f"{self.tile_shape[1]} pixels \n dx = {mx} +- {sx} pixels \n dy = {my} +- {sy} pixels "
                f"\n ({self.method}, best = {self.best})")

    __repr__ = __str__
