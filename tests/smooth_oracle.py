"""
The NaN-aware separable smoothing in numpy -- the only oracle of coreg_smooth_small and its kin.  The rule, stated once
(DESIGN.md section 8): with m = isfinite(v), z = where(m, v, 0) and the tables wy[2 ry + 1], wx[2 rx + 1],

    num = C_y(C_x(z)),  den = C_y(C_x(m as float64))
    C_x(a)[j, i] = sum_k wx[k] a[j, i + k - rx]      (taps outside the image add nothing)
    C_y(a)[j, i] = sum_k wy[k] a[j + k - ry, i]
    out[j, i] = num / den  if m[j, i] and den > 0,  else NaN

float64 throughout, explicit tap loops in rising k, x pass first.
"""
import numpy as np


def _pass(a, w, axis):
    w = np.asarray(w, dtype=np.float64)
    r = len(w) // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(len(w)):
        s = k - r  # out[i] += w[k] a[i + s] for the i with 0 <= i + s < n
        lo, hi = max(0, -s), min(n, n - s)
        if lo >= hi:
            continue
        dst = [slice(None)] * 2
        src = [slice(None)] * 2
        dst[axis] = slice(lo, hi)
        src[axis] = slice(lo + s, hi + s)
        out[tuple(dst)] += w[k] * a[tuple(src)]
    return out


def smooth(v, wy, wx):
    v = np.asarray(v, dtype=np.float64)
    m = np.isfinite(v)
    z = np.where(m, v, 0.0)
    num = _pass(_pass(z, wx, 1), wy, 0)
    den = _pass(_pass(m.astype(np.float64), wx, 1), wy, 0)
    out = np.full(v.shape, np.nan)
    ok = m & (den > 0)
    out[ok] = num[ok] / den[ok]
    return out


def smooth_abs(v, wy, wx):
    """The oracle applied to |v|: the scale of the rounding-error bound of a case."""
    return smooth(np.abs(np.asarray(v, dtype=np.float64)), wy, wx)


def bound(v, wy, wx):
    """|got - want| <= 4 (2 r + 2) 2^-53 want_abs, r the larger reach: each pass is a sum of at most 2 r + 1 products of
    one sign, relative error at most (2 r + 2) u whatever the order or contraction; two passes and a division, and a
    factor 2 of margin."""
    r = max(len(wy), len(wx)) // 2
    return 4.0 * (2 * r + 2) * 2.0 ** -53 * smooth_abs(v, wy, wx)
