"""
CPU oracle of the iterative-context sweep (AlignementSpiceIterativeContextRaster): float64 NumPy / SciPy, independent of
the library (no call into libcoreg_hip).  One lag-point is the reference's `_step` (hdrshift/alignment_spice.py:361-421):

  * headers.  The 4-D SPICE header's celestial part (degrees, CRVAL / CROTA replaced by the flattened header's, the
    *_ref values _shift_header adds the lag to) shifted by `_shift_header` (alignment.py:401-468) gives the grid on
    which the map builder takes the sky positions of the slit pixels (`ctx`); the composed map's header is that grid as
    WCS.to_header prints it, 14 significant digits (`grid`); the flattened header shifted by `_shift_header`, its
    rewritten cards read back from their FITS text (`shifted`).  "reference" semantics: a CDELT1 lag rebuilds PCi_j with
    the unchanged CDELT1, a CDELT2 lag kills the worker (the lag-point stays NaN); "intended": CDELT + lag.
  * context (synras/map_builder.py:89-131): column i is the order-2 sample of the frame col_frame[i] at wcslib's
    pixels of the slit pixels of `ctx`, into an array of the frame's dtype (interpol2d's dst), then float64.
  * SPICE image: order-N sample at wcslib's pixels of `grid` in `shifted`, into float32 (alignment.py:1018-1029).
  * statistics: thresholds on the float32 sample, compared in float32; Pearson masked and means-first
    (c_correlate.py:39-72); 'residus' np.std((a - b) / sqrt(a)) over the thresholded points, no NaN mask.
Coordinates go through coreg_oracle.wcslib_pixel_to_pixel (the C twin of wcslib's TAN arithmetic, built by
oracle/Makefile; the scalar Python restatement otherwise).
"""
import numpy as np
from scipy.ndimage import map_coordinates

from oracle import coreg_oracle as O

INTENDED, REFERENCE = "intended", "reference"
_WCS_KEYS = ("CRPIX1", "CRPIX2", "CRVAL1", "CRVAL2", "CDELT1", "CDELT2", "PC1_1", "PC1_2", "PC2_1", "PC2_2")


def card_float(v):
    """A float as a FITS card holds it and WCS(header) reads it back: f"{v:.16G}", at most 20 characters, the mantissa
    cut before an exponent (astropy's Card formatting)."""
    v = float(v)
    if not np.isfinite(v):
        return v
    s = f"{v:.16G}"
    if "." not in s and "E" not in s:
        s += ".0"
    if len(s) > 20:
        e = s.find("E")
        s = s[:20] if e < 0 else s[:20 - (len(s) - e)] + s[e:]
    return float(s)


def p14(v):
    """wcslib's WCSHDO_P14 (WCS.to_header): 14 significant digits."""
    v = float(v)
    return v if not np.isfinite(v) else float(f"{v:.14G}")


def _crota(hdr):
    return float(hdr["CROTA"] if "CROTA" in hdr else hdr.get("CROTA2", 0.0))


def shift_header(hdr, ref, d_crval1, d_crval2, d_cdelt1, d_cdelt2, d_crota, semantics=INTENDED):
    """alignment.py:401-468 on a copy of `hdr`; `ref` holds the *_ref values (CRVAL, CROTA).  None where the reference's
    worker dies or the header cannot be evaluated (the lag-point stays NaN)."""
    out = dict(hdr)
    out["CRVAL1"] = float(ref["CRVAL1"]) + d_crval1
    out["CRVAL2"] = float(ref["CRVAL2"]) + d_crval2
    change_pcij = False
    if d_cdelt1 != 0.0:
        change_pcij = True
        if semantics == INTENDED:
            out["CDELT1"] = float(hdr["CDELT1"]) + d_cdelt1
        # "reference": the new CDELT1 is computed and never written (alignment.py:421-430)
    if d_cdelt2 != 0.0:
        change_pcij = True
        if semantics != INTENDED:
            return None  # float.to(...) raises inside the worker (alignment.py:440)
        out["CDELT2"] = float(hdr["CDELT2"]) + d_cdelt2
    crot = _crota(ref)
    if d_crota != 0.0:
        change_pcij = True
        crot = _crota(ref) + d_crota
    out["CROTA"] = crot
    with np.errstate(all="ignore"):
        if change_pcij:
            rho = np.deg2rad(np.float64(crot))
            lam = np.float64(out["CDELT2"]) / np.float64(out["CDELT1"])
            out["PC1_1"] = float(np.cos(rho))
            out["PC2_2"] = float(np.cos(rho))
            out["PC1_2"] = float(-lam * np.sin(rho))
            out["PC2_1"] = float((1 / lam) * np.sin(rho))
        vals = [float(out[k]) for k in ("CDELT1", "CDELT2", "CROTA", "PC1_2", "PC2_1")]
    if out["CDELT1"] == 0.0 or out["CDELT2"] == 0.0 or not all(np.isfinite(vals)):
        return None  # astropy refuses such a header: the worker dies
    return out


def lag_headers(target4, hdr_small, d_crval1, d_crval2, d_cdelt1, d_cdelt2, d_crota, semantics=INTENDED):
    """(ctx, grid, shifted) header dicts of one lag-point, or None (see the module docstring).  `target4`: the 4-D
    header's helioprojective cards in degrees; `hdr_small`: the flattened 2-D header (degrees)."""
    def tan(h):
        d = {k: float(h.get(k, 1.0 if k in ("PC1_1", "PC2_2") else 0.0)) for k in _WCS_KEYS}
        d.update(NAXIS1=int(h["NAXIS1"]), NAXIS2=int(h["NAXIS2"]), CROTA=_crota(h), CUNIT1="deg", CUNIT2="deg",
                 CTYPE1="HPLN-TAN", CTYPE2="HPLT-TAN", LONPOLE=float(h.get("LONPOLE", 180.0)))
        return d
    small = tan(hdr_small)
    lag = (float(d_crval1), float(d_crval2), float(d_cdelt1), float(d_cdelt2), float(d_crota))
    ctx = shift_header(tan(target4), small, *lag, semantics=semantics)
    shifted = shift_header(small, small, *lag, semantics=semantics)
    if ctx is None or shifted is None:
        return None
    grid = dict(ctx)
    for k in _WCS_KEYS:
        grid[k] = p14(ctx[k])
    grid["NAXIS1"], grid["NAXIS2"] = small["NAXIS1"], small["NAXIS2"]
    # the cards _shift_header wrote: CRVAL always, CDELT / PCi_j when it rebuilt them
    rewritten = ["CRVAL1", "CRVAL2"] + [k for k in ("CDELT1", "CDELT2") if shifted[k] != small[k]]
    if lag[2] != 0.0 or lag[3] != 0.0 or lag[4] != 0.0:
        rewritten += ["PC1_1", "PC1_2", "PC2_1", "PC2_2"]
    for k in rewritten:
        shifted[k] = card_float(shifted[k])
    return ctx, grid, shifted


def lag_table(lags):
    """The five lag axes (None -> [0.0]) and the C-order list of their combinations."""
    axes = [np.atleast_1d(np.asarray([0.0] if v is None else v, dtype=np.float64)) for v in lags]
    g = np.meshgrid(*axes, indexing="ij")
    return axes, np.stack([a.ravel() for a in g], axis=1)


def context_step(frames, frame_headers, col_frame, spice, target4, hdr_small, lag, order=2, method="correlation",
                 semantics=INTENDED, vmin=None, vmax=None, samples=False):
    """One lag-point: the coefficient (or 'residus'); with `samples`, (value, a, b) where a / b are the context and the
    SPICE sample on the grid (float64, NaN outside), or (NaN, None, None) when the lag-point has no header."""
    r = lag_headers(target4, hdr_small, *lag, semantics=semantics)
    if r is None:
        return (np.nan, None, None) if samples else np.nan
    ctx, grid, shifted = r
    ny, nx = int(hdr_small["NAXIS2"]), int(hdr_small["NAXIS1"])
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    col_frame = np.asarray(col_frame)
    large = np.empty((ny, nx), dtype=np.float64)
    for f in np.unique(col_frame):
        cols = np.nonzero(col_frame == f)[0]
        img = frames[int(f)]
        ox, oy, _, _ = O.wcslib_pixel_to_pixel(ctx, frame_headers[int(f)], xx[:, cols], yy[:, cols])
        dst = np.empty(ox.size, dtype=img.dtype)
        map_coordinates(img, np.stack((oy, ox)), order=2, mode="constant", cval=np.nan, output=dst, prefilter=False)
        large[:, cols] = dst.astype(np.float64).reshape(ny, cols.size)
    ox, oy, _, _ = O.wcslib_pixel_to_pixel(grid, shifted, xx, yy)
    bf = np.empty(ox.size, dtype=np.float32)
    map_coordinates(spice, np.stack((oy, ox)), order=order, mode="constant", cval=np.nan, output=bf, prefilter=False)
    a, b = large.ravel(), bf.astype(np.float64)
    sel = np.ones(a.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        if vmin is not None:
            sel &= bf > np.float32(vmin)
        if vmax is not None:
            sel &= bf < np.float32(vmax)
    with np.errstate(all="ignore"):
        if method == "residus":
            v = float(np.std(((a - b) / np.sqrt(a))[sel])) if sel.any() else np.nan
        elif method == "correlation":
            m = sel & ~np.isnan(a) & ~np.isnan(b)
            v = float(O.c_correlate(a[m], b[m])[0])
        else:
            raise NotImplementedError(method)
    return (v, a, b) if samples else v


def context_sweep(frames, frame_headers, col_frame, spice, target4, hdr_small, lags, order=2, method="correlation",
                  semantics=INTENDED, vmin=None, vmax=None, lag_index=None):
    """The whole sweep, shaped as the five lag axes (NaN where not evaluated); `lag_index` restricts it to those
    C-order lag indices."""
    axes, table = lag_table(lags)
    out = np.full(table.shape[0], np.nan)
    idx = range(table.shape[0]) if lag_index is None else lag_index
    for i in idx:
        out[i] = context_step(frames, frame_headers, col_frame, spice, target4, hdr_small, table[i], order=order,
                              method=method, semantics=semantics, vmin=vmin, vmax=vmax)
    return out.reshape([len(a) for a in axes])
