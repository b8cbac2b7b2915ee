"""
The parameters of the NaN-aware median/MAD despiking (include/coreg_hip.h: coreg_despike_small): what
a `despike_small=` / `despike_large=` keyword becomes before it reaches the library.  No import beyond the standard library:
a bad keyword raises before anything is loaded.
"""
from __future__ import annotations

import math
import numbers

MAX_RADIUS = 3  # csrc/despike_plan.hpp: kDespikeMaxR
MAX_ITER = 8    # kDespikeMaxIter
SIGNS = ("positive", "both")
REPLACES = ("nan", "median")
DEFAULTS = {"radius": 2, "nsigma": 5.0, "floor": 0.0, "min_neighbours": 5, "sign": "positive", "replace": "nan", "n_iter": 2}


def _is_number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _integer(v, name, what, lo, hi):
    if not _is_number(v) or v != int(v) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer from {lo} to {hi} (got {v!r})")
    return int(v)


def despike_params(arg, what="despike"):
    """The parameters of a despiking argument as a dict with every key of `DEFAULTS`; None for None.  True: the defaults
    (5 x 5 window, 5 sigma, two passes, positive spikes only, flagged pixels become NaN); a number: `nsigma`; a dict of any
    of radius (1..3), nsigma (finite, > 0), floor (finite, >= 0), min_neighbours (1..(2 radius + 1)^2 - 1), sign
    ("positive" | "both"), replace ("nan" | "median"), n_iter (1..8).  An unknown key or a value outside its limits raises
    ValueError."""
    if arg is None:
        return None
    err = ValueError(f"{what} must be None, True, a number of sigmas or a dict of {sorted(DEFAULTS)}")
    p = dict(DEFAULTS)
    if arg is True:
        pass
    elif arg is False or isinstance(arg, str):
        raise err
    elif _is_number(arg):
        p["nsigma"] = arg
    elif isinstance(arg, dict):
        unknown = sorted(set(arg) - set(DEFAULTS), key=str)
        if unknown:
            raise ValueError(f"{what}: unknown key(s) {unknown}; known: {sorted(DEFAULTS)}")
        p.update(arg)
    else:
        raise err
    p["radius"] = _integer(p["radius"], "radius", what, 1, MAX_RADIUS)
    p["n_iter"] = _integer(p["n_iter"], "n_iter", what, 1, MAX_ITER)
    p["min_neighbours"] = _integer(p["min_neighbours"], "min_neighbours", what, 1, (2 * p["radius"] + 1) ** 2 - 1)
    for name, positive in (("nsigma", True), ("floor", False)):
        v = p[name]
        if not _is_number(v) or not math.isfinite(v) or v < 0 or (positive and v == 0):
            raise ValueError(f"{what}: {name} must be a finite number {'> 0' if positive else '>= 0'} (got {v!r})")
        p[name] = float(v)
    if p["sign"] not in SIGNS:
        raise ValueError(f"{what}: sign must be one of {SIGNS} (got {p['sign']!r})")
    if p["replace"] not in REPLACES:
        raise ValueError(f"{what}: replace must be one of {REPLACES} (got {p['replace']!r})")
    return p


def despike_planes_params(arg, what="despike_planes"):
    """The parameters of a `despike_planes=` keyword (the wavelength planes of a SPICE window despiked one by one before
    they are summed; include/coreg_hip.h: coreg_despike_sum_planes_be): as `despike_params`, except that True and a bare
    number of sigmas stand for replace="median", not "nan".  A plane pixel set to NaN is a zero term of the sum over the
    planes: where the other planes hold the line, the summed image gets a dip of one plane's worth where the line was, which
    no later step can tell from structure.  The median of the pixel's neighbours in its own plane keeps the term.  A dict
    says what it wants: without a "replace" key it gets `despike_params`' default, "nan"."""
    if arg is True:
        arg = {"replace": "median"}
    elif _is_number(arg):
        arg = {"nsigma": arg, "replace": "median"}
    return despike_params(arg, what)


def despike_tag(p):
    """The parameters as a flat tuple (what names them in the tag of a resident prepared reference); () for None."""
    return () if p is None else ("despike",) + tuple(p[k] for k in sorted(p))
