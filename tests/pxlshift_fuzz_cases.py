"""
Seeded cases of the pxlshift fuzz tests (numpy only; shared by tests/test_pxlshift_fuzz_cpu.py and
tests/test_gpu_pxlshift_fuzz.py).  `case(seed)` draws everything from `np.random.default_rng(seed)` -- no golden file, no
image of another test -- and every structured draw is picked from a named list below, so that the CPU test can assert
that the fixed list `SEEDS` walks every name.

What is varied, and why (csrc/host_pixels.hpp, csrc/kernels_pixels*.hpp):

  lag_dx    the planner cuts the list, in the order given, into runs of at most 16 entries within 16 columns of the run's
            smallest (`groups_of` restates the rule); a slot reads the box at `lag - dx_min`, a group starts at column
            `dx_min - min_dx`.  DX_KINDS: orders, duplicates, strides and lengths at which a run ends for either reason,
            and the two lists [5, 0, 15] (one run whose minimum is not its first entry) and [5, 0, 16] (which must split)
  lag_dy    one workgroup row per entry, `row_off = lag - min_dy`: DY_KINDS
  lag_drot  one plane per entry, 0.0 a copy: DROT_KINDS (equal entries give equal planes)
  shape     SHAPES: the widths and pixel counts at which the staging loops (256 threads), the wave reduction (64 lanes), the
            16 extra box columns and the (row, column) walk of k_pixels_mi (16 or 32 pixels per step, four steps per trip)
            change their path; a 65-row and a 129-row image of width <= 3 are two and three row bands by the 64-row limit
  tiles     TILE_WIDTHS on the column axis, a step that does not divide the tile where the tile allows one, ragged last
            windows
  bins      BINS_KINDS: 256 and 512 threads (the library switches above 16 x 16 cells), na != nb
  pixels    a smoothed random field; NaNs scattered, a full row, a full column; +Inf and -Inf; values <= 0 in the large
            image; weight tables with leading and trailing zeros (an Inf under weight 0)

The branches of the kernels that need more than 16.7 million pixels (the grid stride of k_pixels_resample) or more than
524 280 planes (that of k_pixels_destretch) cannot be reached at test size and are not drawn here.
"""
import numpy as np

from . import pxlshift_oracle as O
from . import pxlshift_windows_oracle as Wd

G = 16  # csrc/kernels_pixels.hpp: kPixG
MAX_LAGS, MAX_WINDOWS = 99, (3, 4)  # per case: lags in all, windows (rows, columns) -- the oracle's Python loops stay short

DX_KINDS = ("contiguous", "descending", "shuffled", "duplicates", "stride2", "stride15", "stride16", "stride17", "len16",
            "len17", "len32", "len33", "negative", "min_last", "min_last_split")
DY_KINDS = ("contiguous", "descending", "shuffled", "duplicates", "single")
DROT_KINDS = ("zero", "zero_twice", "angle_zero_angle")
WIDTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65)
PIXEL_COUNTS = (1, 63, 64, 65, 127, 129, 255, 256, 257, 2047, 2048, 2049)
SHAPES = ((1, 1), (63, 1), (21, 3), (32, 2), (4, 16), (1, 64), (65, 1), (1, 65), (127, 1), (1, 127), (8, 16), (129, 1),
          (43, 3), (17, 15), (15, 17), (16, 16), (8, 32), (4, 64), (257, 1), (1, 257), (89, 23), (23, 89), (64, 32),
          (32, 64), (128, 16), (683, 3), (3, 683), (9, 31), (5, 33), (3, 63), (4, 65), (7, 2), (12, 17), (65, 3), (129, 2))
TILE_WIDTHS = (1, 15, 16, 17, 31, 32, 33)
BINS_KINDS = ("B2", "B16", "B32", "E3_31", "E31_15", "E16_15")
EXPLICIT_EDGES = {"E3_31": (3, 31), "E31_15": (31, 15), "E16_15": (16, 15)}
RATIOS = ((1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (0.5, 0.75), (1.25, 0.5), (0.75, 1.5))  # (ratio_res_1, ratio_res_2)
INF_KINDS = ("none", "none", "none", "large", "large", "small", "both")
TABLE_KINDS = ("gaussian", "zero_ends")

# Picked from the first 1 500 seeds: the fewest that walk every name of `required()` (18 of them), then those that add a
# shape of SHAPES or a dx kind with rotation planes / wide bins not yet walked.  A seed may be swapped for another as long
# as tests/test_pxlshift_fuzz_cpu.py still passes.
SEEDS = (1, 2, 6, 7, 9, 10, 11, 12, 16, 17, 18, 19, 27, 29, 32, 38, 41, 42, 43, 49, 53, 56, 60, 84, 118, 120, 128, 136,
         178, 426, 502, 618, 654, 973, 1064)


def groups_of(lag_dx):
    """[(first, count, dx_min)] of the runs `pixels_sweep_run` cuts a dx list into: entries are taken in order while the
    run holds fewer than 16 and its largest and smallest, the new one included, lie at most 15 apart."""
    dx = [int(v) for v in lag_dx]
    out, i = [], 0
    while i < len(dx):
        lo = hi = dx[i]
        n = 1
        while i + n < len(dx) and n < G:
            v = dx[i + n]
            if max(hi, v) - min(lo, v) > G - 1:
                break
            lo, hi, n = min(lo, v), max(hi, v), n + 1
        out.append((i, n, lo))
        i += n
    return out


def _lag_dx(rng, kind):
    a = int(rng.integers(-4, 4))
    if kind == "contiguous":
        return a + np.arange(int(rng.integers(3, 10)))
    if kind == "descending":
        return (a + np.arange(int(rng.integers(3, 21))))[::-1].copy()
    if kind == "shuffled":
        return rng.permutation(a + np.arange(int(rng.integers(5, 21))))
    if kind == "duplicates":
        v = a + np.arange(18)
        d = v[int(rng.integers(0, 5))]
        head = list(v[:10])
        head.insert(int(rng.integers(5, 10)), d)  # twice in the first run ...
        return np.array(head + list(v[10:]) + [d])  # ... and once more in a later one
    if kind == "stride2":
        return a + 2 * np.arange(int(rng.integers(8, 13)))
    if kind in ("stride15", "stride16", "stride17"):
        return a + int(kind[6:]) * np.arange(int(rng.integers(2, 5)))
    if kind in ("len16", "len17", "len32", "len33"):
        return a + np.arange(int(kind[3:]))
    if kind == "negative":
        return -int(rng.integers(2, 6)) - np.arange(int(rng.integers(3, 9)))[::-1]
    if kind == "min_last":
        return a + np.array([5, 0, 15])
    if kind == "min_last_split":
        return a + np.array([5, 0, 16])
    raise ValueError(kind)


def _lag_dy(rng, kind, n_max):
    b = int(rng.integers(-3, 3))
    if kind == "single":
        return np.array([b])
    if kind == "duplicates":
        return b + np.array([1, 0, 1])
    v = b + np.arange(int(rng.integers(2 if kind != "shuffled" else 3, min(n_max, 5) + 1)))
    if kind == "descending":
        return v[::-1].copy()
    if kind == "shuffled":
        p = rng.permutation(v)
        return p if not np.array_equal(p, v) else v[::-1].copy()
    return v


def _axis(rng, n, sizes, max_windows):
    """(size, step) of the windows along an axis of n pixels: a size from `sizes`, a step that does not divide it where
    one leaves at most `max_windows` windows."""
    fits = []
    for t in sizes:
        steps = [s for s in range(1, t + 1) if (1 if n <= t else -(-(n - t) // s) + 1) <= max_windows]
        if t <= n and steps:
            fits.append((t, steps))
    t, steps = fits[int(rng.integers(0, len(fits)))]
    odd = [s for s in steps if t % s]
    steps = odd or steps
    return int(t), int(steps[int(rng.integers(0, len(steps)))])


def _table(rng, n, kind):
    if kind == "gaussian":
        return Wd.gaussian_table(n, n / 4.0)
    t = rng.uniform(0.2, 1.0, n)
    if n >= 4:
        t[0] = t[-1] = 0.0
    if n >= 7:
        t[1] = 0.0
    return t


def _edges(rng, n, lo, hi):
    while True:
        e = np.sort(rng.uniform(lo, hi, n))
        if np.all(np.diff(e) > 0):
            return e


def case(seed):
    """A dict of plain arrays and arguments: large, small, hdr_large, hdr_small, lag_dx, lag_dy, lag_drot, tile_shape,
    tile_step, window (the two weight tables), bins (an integer or a pair of edge lists), and `kinds`: the names drawn and
    what was put into the pixels, for the coverage assertions."""
    rng = np.random.default_rng(seed)
    kinds = {}
    h, w = SHAPES[int(rng.integers(0, len(SHAPES)))]
    kinds["dx"] = DX_KINDS[int(rng.integers(0, len(DX_KINDS)))]
    lag_dx = _lag_dx(rng, kinds["dx"])
    # rotation planes, then dy lags, as the budget of lags allows
    rot_ok = [k for k, n in zip(DROT_KINDS, (1, 2, 3)) if n * len(lag_dx) <= MAX_LAGS]
    kinds["drot"] = rot_ok[int(rng.integers(0, len(rot_ok)))]
    angle = float(rng.uniform(0.5, 3.0)) * (1 if rng.random() < 0.5 else -1)  # degrees
    lag_drot = {"zero": np.array([0.0]), "zero_twice": np.array([0.0, 0.0]),
                "angle_zero_angle": np.array([angle, 0.0, angle])}[kinds["drot"]]
    n_dy = MAX_LAGS // (len(lag_dx) * len(lag_drot))
    dy_ok = [k for k in DY_KINDS if n_dy >= {"single": 1, "contiguous": 2, "descending": 2}.get(k, 3)]
    kinds["dy"] = dy_ok[int(rng.integers(0, len(dy_ok)))]
    lag_dy = _lag_dy(rng, kinds["dy"], n_dy)

    # the large image: a smoothed field under which every lag stays inside
    r1, r2 = RATIOS[int(rng.integers(0, len(RATIOS)))]
    kinds["ratio"] = (r1, r2)
    mx, my = int(np.abs(lag_dx).max()), int(np.abs(lag_dy).max())
    H, W = int(np.ceil((h + 2 * my + 2) * r2)) + 1, int(np.ceil((w + 2 * mx + 2) * r1)) + 1
    raw = rng.uniform(1.0, 9.0, (H, W))
    large = sum(np.roll(np.roll(raw, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    sub = O.sub_resolution(large, r1, r2)
    l = O.slice_origin(sub.shape, (h, w))
    tdx, tdy = int(lag_dx[int(rng.integers(0, len(lag_dx)))]), int(lag_dy[int(rng.integers(0, len(lag_dy)))])
    small = sub[l[0] + tdy:l[0] + tdy + h, l[1] + tdx:l[1] + tdx + w] + rng.normal(0.0, 0.05, (h, w))
    assert small.shape == (h, w) and np.isfinite(small).all()

    # tiles, steps, weight tables
    # (no width of TILE_WIDTHS leaves an image wider than 99 pixels in four windows or fewer: a third of it or more does)
    widths = TILE_WIDTHS + (tuple(range(-(-w // 3), w + 1)) if w > 99 else (w,))
    tw, sx = _axis(rng, w, widths, MAX_WINDOWS[1])
    th, sy = _axis(rng, h, tuple(range(max(1, -(-h // 3)), h + 1)), MAX_WINDOWS[0])
    kinds["tile_width"] = tw
    kinds["table"] = TABLE_KINDS[int(rng.integers(0, len(TABLE_KINDS)))]
    window = (_table(rng, th, kinds["table"]), _table(rng, tw, kinds["table"]))

    # bins: a number needs quantiles of both images, explicit edges do not
    pick = BINS_KINDS if h * w >= 32 else tuple(EXPLICIT_EDGES)
    kinds["bins"] = pick[int(rng.integers(0, len(pick)))]
    if kinds["bins"] in EXPLICIT_EDGES:
        ns, nl = EXPLICIT_EDGES[kinds["bins"]]
        bins = (_edges(rng, ns, 2.0, 8.0), _edges(rng, nl, 2.0, 8.0))
    else:
        bins = int(kinds["bins"][1:])

    # what goes into the pixels
    def to_large(r, c):  # the pixel of the large image at row r, column c of the sub-resolved one
        return min(H - 1, int(round(r * r2))), min(W - 1, int(round(c * r1)))

    n_small, n_large = h * w // 40, H * W // 60
    small[rng.integers(0, h, n_small), rng.integers(0, w, n_small)] = np.nan
    large[rng.integers(0, H, n_large), rng.integers(0, W, n_large)] = np.nan
    kinds["nan_row_small"] = bool(h >= 4 and rng.random() < 0.25)
    kinds["nan_col_small"] = bool(w >= 4 and rng.random() < 0.25)
    kinds["nan_row_large"] = bool(h >= 4 and rng.random() < 0.25)
    kinds["nan_col_large"] = bool(w >= 4 and rng.random() < 0.25)
    if kinds["nan_row_small"]:
        small[int(rng.integers(0, h)), :] = np.nan
    if kinds["nan_col_small"]:
        small[:, int(rng.integers(0, w))] = np.nan
    if kinds["nan_row_large"]:
        large[to_large(l[0] + int(rng.integers(0, h)), 0)[0], :] = np.nan
    if kinds["nan_col_large"]:
        large[:, to_large(0, l[1] + int(rng.integers(0, w)))[1]] = np.nan
    kinds["nonpositive"] = bool(rng.random() < 0.3)
    if kinds["nonpositive"]:  # under the small image at lag (0, 0): one zero, one negative pixel
        for v in (0.0, -1.5):
            large[to_large(l[0] + int(rng.integers(0, h)), l[1] + int(rng.integers(0, w)))] = v
    kinds["inf"] = INF_KINDS[int(rng.integers(0, len(INF_KINDS)))]
    if kinds["inf"] in ("large", "both"):  # the two far corners of what the lags reach: a few lags see each
        large[to_large(l[0] + int(lag_dy.max()) + h - 1, l[1] + int(lag_dx.max()) + w - 1)] = np.inf
        large[to_large(l[0] + int(lag_dy.min()), l[1] + int(lag_dx.min()))] = -np.inf
    inf_small = []
    if kinds["inf"] in ("small", "both"):  # row 0: under a zero of a table with zero ends
        inf_small = [(0, int(rng.integers(0, w)), np.inf), (h - 1, int(rng.integers(0, w)), -np.inf)]
        for r, c, v in inf_small:
            small[r, c] = v
    slices = Wd.window_slices((h, w), (th, tw), (sy, sx))
    kinds["inf_under_zero_weight"] = any(
        rs.start <= r < rs.stop and cs.start <= c < cs.stop and window[0][r - rs.start] * window[1][c - cs.start] == 0.0
        for r, c, _ in inf_small for row in slices for rs, cs in row)
    last_r, last_c = slices[-1][-1]
    kinds["ragged"] = (last_r.stop - last_r.start < th, last_c.stop - last_c.start < tw)
    hdr = {"CDELT1": 1.0, "CDELT2": 1.0, "CUNIT1": "arcsec", "CUNIT2": "arcsec"}
    return {"seed": seed, "large": large, "small": small, "hdr_large": dict(hdr),
            "hdr_small": dict(hdr, CDELT1=r1, CDELT2=r2), "lag_dx": lag_dx.astype(np.int64),
            "lag_dy": lag_dy.astype(np.int64), "lag_drot": lag_drot, "tile_shape": (th, tw), "tile_step": (sy, sx),
            "window": window, "bins": bins, "kinds": kinds}


def marks(c):
    """The names a case walks, as a set of tuples: what the coverage test counts over `SEEDS`."""
    k = c["kinds"]
    h, w = c["small"].shape
    (th, tw), (sy, sx) = c["tile_shape"], c["tile_step"]
    out = {("dx", k["dx"]), ("dy", k["dy"]), ("drot", k["drot"]), ("bins", k["bins"]), ("table", k["table"]),
           ("width", w), ("pixels", h * w), ("tile_width", tw)}
    if w <= 3 and h in (65, 129):
        out.add(("row_bands", -(-h // 64)))
    if th % sy or tw % sx:
        out.add(("step_not_dividing",))
    out |= {(name,) for name, on in zip(("ragged_rows", "ragged_columns"), k["ragged"]) if on}
    out |= {(name,) for name in ("nan_row_small", "nan_col_small", "nan_row_large", "nan_col_large", "nonpositive",
                                 "inf_under_zero_weight") if k[name]}
    out |= {("inf", where) for where in ("large", "small") if k["inf"] in (where, "both")}
    if k["ratio"][0] != k["ratio"][1] and 1.0 not in k["ratio"]:
        out.add(("ratio", "unequal_non_unit"))
    if np.isnan(c["small"]).any() and np.isnan(c["large"]).any():
        out.add(("nan_scattered",))
    dx = [int(v) for v in c["lag_dx"]]
    runs = groups_of(dx)
    for n, (first, count, lo) in enumerate(runs):
        if count == G:
            out.add(("run_of_16",))
            if n + 1 < len(runs) and runs[n + 1][1] == 1:
                out.add(("run_of_1_after_16",))
        if dx[first] != lo:
            out.add(("run_min_not_first",))
        if len(set(dx[first:first + count])) < count:
            out.add(("run_with_duplicate",))
    seen = {}
    for n, (first, count, _) in enumerate(runs):
        for v in dx[first:first + count]:
            seen.setdefault(v, set()).add(n)
    if any(len(s) > 1 for s in seen.values()):
        out.add(("duplicate_in_two_runs",))
    return out


def required():
    """Every mark the seed list has to walk at least once."""
    need = {("dx", v) for v in DX_KINDS} | {("dy", v) for v in DY_KINDS} | {("drot", v) for v in DROT_KINDS}
    need |= {("bins", v) for v in BINS_KINDS} | {("table", v) for v in TABLE_KINDS}
    need |= {("width", v) for v in WIDTHS} | {("pixels", v) for v in PIXEL_COUNTS} | {("tile_width", v) for v in TILE_WIDTHS}
    need |= {("row_bands", 2), ("row_bands", 3), ("inf", "large"), ("inf", "small"), ("ratio", "unequal_non_unit")}
    need |= {(v,) for v in ("step_not_dividing", "ragged_rows", "ragged_columns", "nan_row_small", "nan_col_small",
                            "nan_row_large", "nan_col_large", "nonpositive", "inf_under_zero_weight", "nan_scattered",
                            "run_of_16", "run_of_1_after_16", "run_min_not_first", "run_with_duplicate",
                            "duplicate_in_two_runs")}
    return need
