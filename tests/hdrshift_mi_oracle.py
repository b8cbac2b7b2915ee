"""numpy oracle of the mutual-information score of the Carrington header-shift sweep (include/coreg_hip.h:
coreg_sweep_set_bins), composed like tests/masked_scores_oracle.py from the CPU oracle's own building blocks
(oracle/coreg_oracle.py: set_initial_header_values, lag_table, prepare_reference, shift_header, carrington_transform_fa,
carrington_coords) plus tests/pxlshift_mi_oracle.py's score of a finished histogram.  For every lag-point:

  A = reference image on the target grid, B = resampled image to align, mask = isfinite(A) & isfinite(B)
  i = np.searchsorted(edges_small, B[mask], side="right"), j = np.searchsorted(edges_large, A[mask], side="right")
  n_ij = np.add.at over (i, j);  MI = mi_of_histogram(n_ij) in nats, NaN for an empty mask;  count = mask.sum()

The mask is the Pearson sums' (an infinite value is dropped; the pixel-lag sweep's oracle keeps it)."""
import numpy as np

from oracle import coreg_oracle as O
from tests.pxlshift_mi_oracle import mi_of_histogram


def histogram(A, B, edges_small, edges_large):
    """The joint histogram [len(edges_small) + 1][len(edges_large) + 1] (int64): rows the bins of B, columns those of A."""
    a, b = np.asarray(A, dtype=np.float64).ravel(), np.asarray(B, dtype=np.float64).ravel()
    mask = np.isfinite(a) & np.isfinite(b)
    i = np.searchsorted(np.asarray(edges_small, dtype=np.float64), b[mask], side="right")
    j = np.searchsorted(np.asarray(edges_large, dtype=np.float64), a[mask], side="right")
    hist = np.zeros((len(edges_small) + 1, len(edges_large) + 1), dtype=np.int64)
    np.add.at(hist, (i, j), 1)
    return hist


def _lag_points(st):
    """(index, solar_r index, A, shifted header, solar_r) of every lag-point of a Carrington sweep of `st`; the shape."""
    O.set_initial_header_values(st, True)
    table, shp = O.lag_table(st)

    def walk():
        for kk, d_solar_r in enumerate(st.lag_solar_r):
            A = O.prepare_reference(st, "carrington", d_solar_r, True)
            for i, lg in enumerate(table):
                hdr = dict(st.hdr_small)
                O.shift_header(st, hdr, *lg)
                yield i, kk, A, hdr, d_solar_r
    return walk(), table.shape[0], shp


def sweep(st, frame, edges_small, edges_large):
    """The whole sweep of `st` (tests/helpers.oracle_state): {"mi", "count"}, 6-D arrays [crval1, crval2, cdelt1, cdelt2,
    crota, solar_r].  frame: "carrington" (the only frame that has the score)."""
    assert frame == "carrington"
    walk, n, shp = _lag_points(st)
    nsr = len(st.lag_solar_r)
    out = {k: np.full((n, nsr), np.nan) for k in ("mi", "count")}
    for i, kk, A, hdr, d_solar_r in walk:
        B = O.carrington_transform_fa(st.data_small, hdr, d_solar_r, st.shape, st.lonlims, st.latlims, st.order)
        hist = histogram(A, B, edges_small, edges_large)
        out["mi"][i, kk], out["count"][i, kk] = mi_of_histogram(hist), int(hist.sum())
    return {k: v.reshape(shp + (nsr,)) for k, v in out.items()}


def _edge_distance(v, edges):
    """The smallest |v - e| / max(|v|, |e|) over the values and the edges (inf without a value)."""
    v = np.asarray(v, dtype=np.float64).ravel()
    e = np.asarray(edges, dtype=np.float64)
    if v.size == 0:
        return np.inf
    d = np.abs(v[:, None] - e[None, :])
    scale = np.maximum(np.abs(v)[:, None], np.abs(e)[None, :])
    return float(np.where(d == 0.0, 0.0, d / np.where(scale > 0.0, scale, 1.0)).min())


def margins(st, edges_small, edges_large):
    """(edge, bound): the smallest relative distance of any kept A or B value of the sweep to an edge of its list, and the
    smallest distance in pixels of any finite sample coordinate to a bound of the image to align (0 and n - 1 on either
    axis).  A comparison against another implementation of the same arithmetic is only meaningful when both are far
    above the rounding of a value (1e-16 relative) and of a coordinate (1e-12 px)."""
    walk, _, _ = _lag_points(st)
    ny, nx = st.data_small.shape
    edge, bound = np.inf, np.inf
    for _, _, A, hdr, d_solar_r in walk:
        cx, cy = O.carrington_coords(hdr, d_solar_r, st.shape, st.lonlims, st.latlims)
        fin = np.isfinite(cx) & np.isfinite(cy)
        for c, n in ((cx[fin], nx), (cy[fin], ny)):
            if c.size:
                bound = min(bound, float(np.abs(c).min()), float(np.abs(c - (n - 1)).min()))
        B = O.interpol2d(st.data_small, cx, cy, fill=-32762, order=st.order)
        B = np.where(B == -32762, np.nan, B)
        mask = np.isfinite(A) & np.isfinite(B)
        edge = min(edge, _edge_distance(B[mask], edges_small), _edge_distance(A[mask], edges_large))
    return edge, bound
