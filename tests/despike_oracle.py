"""
The NaN-aware median/MAD despiking in numpy -- the only oracle of coreg_despike_small and its kin.  The rule, stated once
(include/coreg_hip.h), for every finite pixel v[j, i] of a pass's input:

    N     = the finite pixels of the window [j-R, j+R] x [i-R, i+R] clipped to the image, centre left out, as float64
    k     = |N|;  k < min_neighbours: kept
    med   = s[k/2] for odd k, else (s[k/2 - 1] + s[k/2]) * 0.5,  s = N sorted ascending
    mad   = the same selection over |n - med|
    scale = max(1.4826 * mad, floor);  d = v - med
    flagged when scale > 0 and d > nsigma * scale   (sign = "both": |d| > nsigma * scale)
    flagged -> NaN   (replace = "median": med, rounded to the image's dtype)

Explicit sorts and the explicit (a + b) * 0.5, one pixel at a time: no library median.  All decisions of a pass are taken on
its input; n_iter passes run, each on the result of the one before.
"""
import numpy as np

DEFAULTS = dict(radius=2, nsigma=5.0, floor=0.0, min_neighbours=5, sign="positive", replace="nan", n_iter=2)


def _middle(values):
    s = np.sort(np.asarray(values, dtype=np.float64))
    k = len(s)
    if k % 2:
        return s[k // 2]
    return (s[k // 2 - 1] + s[k // 2]) * np.float64(0.5)


def despike_pass(v, radius=2, nsigma=5.0, floor=0.0, min_neighbours=5, sign="positive", replace="nan"):
    """One pass: (result of v's dtype, number of pixels flagged)."""
    v = np.asarray(v)
    assert v.ndim == 2 and v.dtype in (np.float32, np.float64)
    H, W = v.shape
    R = int(radius)
    v64 = v.astype(np.float64)
    finite = np.isfinite(v64)
    out = v.copy()
    nsigma, floor = np.float64(nsigma), np.float64(floor)
    n_flagged = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(H):
            j0, j1 = max(0, j - R), min(H, j + R + 1)
            for i in range(W):
                if not finite[j, i]:
                    continue
                i0, i1 = max(0, i - R), min(W, i + R + 1)
                take = finite[j0:j1, i0:i1].copy()
                take[j - j0, i - i0] = False
                N = v64[j0:j1, i0:i1][take]
                if len(N) < min_neighbours:
                    continue
                med = _middle(N)
                mad = _middle(np.abs(N - med))
                scale = max(np.float64(1.4826) * mad, floor)
                d = v64[j, i] - med
                lim = nsigma * scale
                if scale > 0 and (abs(d) > lim if sign == "both" else d > lim):
                    n_flagged += 1
                    out[j, i] = v.dtype.type(med) if replace == "median" else np.nan
    return out, n_flagged


def despike(v, n_iter=2, **rule):
    """n_iter passes: (result of v's dtype, [pixels flagged per pass])."""
    out = np.asarray(v)
    counts = []
    for _ in range(int(n_iter)):
        out, n = despike_pass(out, **rule)
        counts.append(n)
    return out, counts


def scene(dtype=np.float64, seed=5):
    """The seeded 96 x 128 scene of the issue: (image of `dtype` with spikes and a NaN block, truth, mask of raised pixels)."""
    rng = np.random.default_rng(seed)
    H, W = 96, 128
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = 200.0 + 150.0 * np.sin(x / 7.0) * np.cos(y / 9.0) + 80.0 * np.exp(-((x - 60.0) ** 2 + (y - 40.0) ** 2) / 50.0)
    img = rng.poisson(truth).astype(np.float64)
    flat = rng.choice(H * (W - 1), size=150, replace=False)  # (a raised pixel always has a right-hand neighbour)
    jj, ii = flat // (W - 1), flat % (W - 1)
    raised = np.zeros((H, W), dtype=bool)
    img[jj, ii] += rng.uniform(300.0, 5000.0, size=150)
    raised[jj, ii] = True
    img[jj[:30], ii[:30] + 1] += 800.0
    raised[jj[:30], ii[:30] + 1] = True
    img[10:14, 100:105] = np.nan
    raised[10:14, 100:105] = False
    return img.astype(dtype), truth, raised


def pearson(a, b):
    """Masked Pearson coefficient of two images over the pixels finite in both."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok] - a[ok].mean(), b[ok] - b[ok].mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
