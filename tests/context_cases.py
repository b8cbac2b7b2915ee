"""Seeded synthetic scenes of the iterative-context sweep (shared by tests/test_context_oracle_cpu.py and
tests/test_gpu_context_fuzz.py): imager frames with TAN headers rendered from one blob field (synthetic.make_scene's
renderer), a SPICE raster header in degrees, its 4-D celestial target, the frame of every column, five lag axes (in
the header's unit, degrees) and the sweep's options.  Every case is a plain dict; `oracle(case)` evaluates it with
oracle/context_oracle.py, `gpu(handle, case)` through coreg_set_context_frames / coreg_set_small / coreg_sweep_context."""
import numpy as np

from euispice_coreg_amd import synthetic
from oracle import context_oracle as CO

AS = 1.0 / 3600.0  # arcsec in degrees


def tan_header(nx, ny, crpix, crval_deg, cdelt_deg, crota):
    """A helioprojective TAN header in degrees, PCi_j from CROTA (alignment.py:462-468), 14 significant digits."""
    h = synthetic._header(nx, ny, crpix[0], crpix[1], crval_deg[0], crval_deg[1], cdelt_deg[0], cdelt_deg[1], crota,
                          unit="deg")
    for k in ("CRPIX1", "CRPIX2", "CRVAL1", "CRVAL2", "CDELT1", "CDELT2", "PC1_1", "PC1_2", "PC2_1", "PC2_2"):
        h[k] = CO.p14(h[k])
    return h


def blobs(rng, centre, half, n=60):
    b = np.empty((n, 4))
    b[:, 0] = centre[0] + rng.uniform(-half, half, n)
    b[:, 1] = centre[1] + rng.uniform(-half, half, n)
    b[:, 2] = rng.uniform(4.0, 30.0, n)
    b[:, 3] = np.exp(rng.uniform(np.log(50.0), np.log(2000.0), n))
    return b


def render(hdr, field, rng):
    return synthetic._render(hdr, field, 100.0, rng)


def make_case(seed, gW=None, gH=None, method=None, order=None, semantics=None, frame_dtype=None, spice_dtype=None,
              n_frames=None, col_mode=None, thresholds=None, nan_frac=None, zeros=None, lags=None):
    """One seeded scene; every dimension drawn from the seed unless given."""
    rng = np.random.default_rng(seed)
    pick = lambda v, choices: choices[rng.integers(len(choices))] if v is None else v  # noqa: E731
    gW = int(pick(gW, [1, 2, 3, int(rng.integers(2, 7)) * 2 + 1, int(rng.integers(2, 7)) * 2]))
    gH = int(pick(gH, [1, 7, 100, 128, 300]))
    method = pick(method, ["correlation", "correlation", "residus"])
    order = int(pick(order, [0, 2, 2, 4]))
    semantics = pick(semantics, [CO.INTENDED, CO.REFERENCE])
    frame_dtype = np.dtype(pick(frame_dtype, [np.float32, np.float64]))
    spice_dtype = np.dtype(pick(spice_dtype, [np.float32, np.float64]))
    n_frames = int(pick(n_frames, [1, 2, 3, 5, 8]))
    col_mode = pick(col_mode, ["one", "blocks", "every", "random"])
    thresholds = pick(thresholds, ["none", "min", "max", "both"])
    # SPICE raster: ~4" steps across the slit, ~1.1" along it; rotated, sometimes a negative CDELT1, CRPIX off-centre
    true_c = np.array([-310.0, 420.0]) + rng.uniform(-30, 30, 2)
    cd1 = rng.uniform(3.5, 4.5) * (-1 if rng.random() < 0.3 else 1)
    cd2 = rng.uniform(1.0, 1.2)
    crota = rng.uniform(-8.0, 8.0) if rng.random() < 0.8 else 0.0
    crpix = ((gW + 1) / 2.0, (gH + 1) / 2.0)
    if rng.random() < 0.5:
        crpix = (crpix[0] + rng.uniform(-0.4 * gW - 2, 0.4 * gW + 2), crpix[1] + rng.uniform(-0.3 * gH - 2, 0.3 * gH + 2))
    err = rng.uniform(-6, 6, 2)
    hdr_small = tan_header(gW, gH, crpix, ((true_c[0] - err[0]) * AS, (true_c[1] - err[1]) * AS), (cd1 * AS, cd2 * AS),
                           crota)
    hdr_true = dict(hdr_small, CRVAL1=true_c[0] * AS, CRVAL2=true_c[1] * AS)
    # the 4-D header's celestial cards: the flattened header's, unrounded; now and then CRPIX a quarter pixel away
    target4 = dict(hdr_small)
    target4["CDELT1"] = cd1 * AS
    target4["CDELT2"] = cd2 * AS
    if rng.random() < 0.3:
        target4["CRPIX1"] = hdr_small["CRPIX1"] + 0.25
    half = 0.5 * max(abs(cd1) * gW, cd2 * gH) + 120.0
    field = blobs(rng, true_c, half)
    # imager frames: an FSI-like 3"/px TAN grid around the raster, each with its own small pointing jitter and rotation
    fn = int(rng.integers(72, 112))
    frames, frame_headers = [], []
    for _ in range(n_frames):
        fc = true_c + rng.uniform(-20, 20, 2)
        hf = synthetic._header(fn, fn, (fn + 1) / 2.0 + rng.uniform(-3, 3), (fn + 1) / 2.0 + rng.uniform(-3, 3),
                               fc[0], fc[1], 3.0 + rng.uniform(-0.2, 0.2), 3.0 + rng.uniform(-0.2, 0.2),
                               rng.uniform(-4, 4), unit="arcsec")
        img = render(hf, field, rng)
        frames.append(img)
        frame_headers.append(hf)
    spice = render(hdr_true, field, rng) * rng.uniform(0.5, 2.0)
    nan_frac = (0.0 if method == "residus" else float(pick(None, [0.0, 0.0, 0.01, 0.05]))) if nan_frac is None \
        else nan_frac
    if nan_frac > 0:
        for img in frames:
            img[rng.random(img.shape) < nan_frac] = np.nan
        spice[rng.random(spice.shape) < nan_frac] = np.nan
    zeros = (method == "residus" and rng.random() < 0.5) if zeros is None else zeros
    if zeros:  # zeros and negatives in the frames (masked corners, over-subtracted dark)
        for img in frames:
            m = rng.random(img.shape)
            img[m < 0.02] = 0.0
            img[(m >= 0.02) & (m < 0.03)] *= -1.0
    frames = [f.astype(frame_dtype) for f in frames]
    spice = spice.astype(spice_dtype)
    col_frame = {"one": np.zeros(gW, dtype=np.int64),
                 "blocks": np.minimum(np.arange(gW) * n_frames // max(gW, 1), n_frames - 1),
                 "every": np.arange(gW) % n_frames,
                 "random": rng.integers(0, n_frames, gW)}[col_mode].astype(np.int64)
    finite = spice[np.isfinite(spice)]
    vmin = float(np.quantile(finite, rng.uniform(0.1, 0.5))) if thresholds in ("min", "both") else None
    vmax = float(np.quantile(finite, rng.uniform(0.6, 0.95))) if thresholds in ("max", "both") else None
    if lags is None:
        lags = lag_axes(rng, semantics)
    return dict(seed=seed, frames=frames, frame_headers=frame_headers, col_frame=col_frame, spice=spice,
                target4=target4, hdr_small=hdr_small, lags=lags, order=order, method=method, semantics=semantics,
                vmin=vmin, vmax=vmax)


def lag_axes(rng, semantics):
    """Five lag axes (degrees): single-valued, descending, holding an exact 0, CDELT2 lags (NaN lag-points under the
    reference's semantics), shifts that move the grid partly or wholly off the frames."""
    kind = rng.integers(6)
    c1 = np.sort(rng.uniform(-8, 8, int(rng.integers(1, 6))))
    c2 = np.sort(rng.uniform(-8, 8, int(rng.integers(1, 5))))[::-1]  # descending
    if kind == 0:
        c1 = np.array([0.0])
    elif kind == 1:
        c1 = np.array([-6.0, 0.0, 6.0])
    elif kind == 2:  # partly / wholly off the frames (~120-160" from the raster to the frame edge)
        c1 = np.array([-400.0, -150.0, 0.0, 140.0])
    cd1 = None if rng.random() < 0.5 else np.array([0.0, rng.uniform(0.05, 0.3)])
    cd2 = None if rng.random() < 0.5 else np.array([rng.uniform(-0.05, -0.01), 0.0])
    cr = None if rng.random() < 0.4 else np.array([0.0, rng.uniform(-1.5, 1.5)])[::int(rng.choice([-1, 1]))]
    ax = [c1, c2, cd1, cd2, cr]
    n = int(np.prod([1 if v is None else len(v) for v in ax]))
    while n > 64:  # keep the oracle's share of a case to a second or two
        k = int(np.argmax([0 if v is None else len(v) for v in ax]))
        ax[k] = ax[k][::2]
        n = int(np.prod([1 if v is None else len(v) for v in ax]))
    return [None if v is None else np.asarray(v, dtype=np.float64) * (AS if k < 4 else 1.0) for k, v in enumerate(ax)]


def oracle(case, lag_index=None):
    return CO.context_sweep(case["frames"], case["frame_headers"], case["col_frame"], case["spice"], case["target4"],
                            case["hdr_small"], case["lags"], order=case["order"], method=case["method"],
                            semantics=case["semantics"], vmin=case["vmin"], vmax=case["vmax"], lag_index=lag_index)


def upload(h, case):
    h.reference_tag = None
    h.set_context_frames(case["frames"], case["frame_headers"])
    h.set_small(case["spice"])


def gpu(h, case, upload_first=True, **kw):
    """The sweep through the handle (shaped as the lag axes when the whole sweep is asked for)."""
    from euispice_coreg_amd import _lib
    if upload_first:
        upload(h, case)
    ls = _lib.LagSet(*case["lags"])
    out = h.sweep_context(case["target4"], case["hdr_small"], case["col_frame"], ls, order=case["order"],
                          method=_lib.METHOD_RESIDUS if case["method"] == "residus" else _lib.METHOD_CORRELATION,
                          cdelt_semantics=_lib.CDELT_INTENDED if case["semantics"] == CO.INTENDED else
                          _lib.CDELT_REFERENCE, vmin=case["vmin"], vmax=case["vmax"], **kw)
    return out.reshape(ls.shape) if not kw else out
