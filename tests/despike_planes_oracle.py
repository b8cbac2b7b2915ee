"""
coreg_despike_sum_planes_be in numpy, on top of tests/despike_oracle.py -- the only oracle of the call (include/coreg_hip.h
states the contract):

    every plane of the stack [n_sel][H][W], in the order given, is despiked on its own: n_iter passes of
    despike_oracle.despike_pass, each on the result of the one before, the window inside the plane;
    sum    = np.nansum(float64(despiked stack), axis=0): a sequential float64 accumulation over the planes from +0.0, a NaN
             a zero term, +-Inf passing through;
    events = flag events per pixel over all passes and planes (int32);  counts[p] = flag events of pass p.
"""
import numpy as np

from tests import despike_oracle as DO


def despike_sum_planes(stack, n_iter=2, **rule):
    """(sum float64 [H, W], events int32 [H, W], [flag events per pass]) of a stack [n_sel, H, W] of float32 / float64."""
    stack = np.asarray(stack)
    assert stack.ndim == 3 and stack.dtype in (np.float32, np.float64)
    n_iter = int(n_iter)
    events = np.zeros(stack.shape[1:], dtype=np.int32)
    counts = [0] * n_iter
    despiked = np.empty(stack.shape, dtype=stack.dtype)
    for k, plane in enumerate(stack):
        out = plane
        for p in range(n_iter):
            new, n = DO.despike_pass(out, **rule)
            # a flag event changes the pixel (finite -> NaN, or -> the median, which differs from it: d > 0 or |d| > 0)
            changed = ~((new == out) | (np.isnan(new) & np.isnan(out)))
            assert int(changed.sum()) == n
            events += changed
            counts[p] += n
            out = new
        despiked[k] = out
    total = np.zeros(stack.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for plane in despiked:  # (np.nansum over the outer axis adds the planes one after another: asserted below)
            term = plane.astype(np.float64)
            total = total + np.where(np.isnan(term), 0.0, term)
        if len(despiked):
            assert np.array_equal(total, np.nansum(despiked.astype(np.float64), axis=0), equal_nan=True)
    return total, events, counts


def be(stack):
    """The stack as a FITS data unit stores it: big-endian, same values."""
    stack = np.asarray(stack)
    return stack.astype(stack.dtype.newbyteorder(">"))
