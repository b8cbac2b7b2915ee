"""
What a closed handle leaves behind on the device, and that closing is safe at any time ("Ownership").

A cycle creates a handle, makes it reserve every family of buffers it has -- a helioprojective sweep at order 3 (the nine
single-sample lists tap_*), a Carrington sweep under differential rotation (t_lon_deg, t_dx), a pixel-lag sweep
(PixelsState), an iterative-context sweep (ContextState) -- and closes it.  After two warm-up cycles (code objects, the
runtime's pools and torch's context are then in place) the device memory in use is read, then again after each of six
more cycles.

Bound: the smallest of the last three readings minus the reading after the warm-up is below 20 MiB.  That is no
measurement but the size of ONE allocation a closed handle used to keep, tap_segq: 2^20 * 16 bytes grown by DevBuf's 25 % +
256 B, reserved by every helioprojective sweep; one lost handle's worth fails the test, six are 120 MiB.  The reading
(torch.cuda.mem_get_info) is device-wide, hence the minimum of three and not the last one.

Measured on one MI355X: with the hand-written release lists the readings were 22, 46, 68, 90, 114, 136 MiB above the
warm-up, for the handle and for the multi-device handle alike (the test's figure is then the reading after the fourth
cycle, 90 MiB); now 0.0 MiB after every cycle.
"""
import gc

import numpy as np
import pytest
import torch

from euispice_coreg_amd import _lib
from euispice_coreg_amd.pxlshift import AlignmentPixels

from . import context_cases as CC
from . import helpers as H
from . import pxlshift_mi_oracle as M
from .pxlshift_tiles_cases import HDR

pytestmark = pytest.mark.gpu

BOUND = 20 * 2 ** 20
assert BOUND < 2 ** 20 * 16 * 5 // 4 + 256  # (tap_segq as DevBuf::reserve sizes it)
LAGS = (17.0 + 2.0 * (np.arange(3) - 1), -9.0 + 2.0 * (np.arange(3) - 1), None, None, None)
ROT = (2.0, 14.51, -3.12, 0.34)  # days, then the three coefficients in degrees per day


@pytest.fixture(scope="module")
def inputs():
    small, hs, large, hl, _ = H.scene(small_n=64, large_n=96)
    assert small.shape == (64, 64) and large.shape == (96, 96)
    pl, ps, _ = M.scene(seed=1, shape=(24, 20), lag=(-1, 1))
    A = AlignmentPixels((pl, dict(HDR)), 0, (ps, dict(HDR)), 0)
    plan = A.host_plan(lag_dx=np.arange(-1, 2), lag_dy=np.arange(-1, 2), lag_drot=np.array([0.0]))
    ctx = CC.make_case(7, gW=5, gH=7, method="correlation", order=2, n_frames=2, col_mode="every", thresholds="none",
                       nan_frac=0.0, lags=[np.array([-2.0, 0.0, 2.0]) * CC.AS, np.array([-2.0, 0.0, 2.0]) * CC.AS, None,
                                           None, None])
    return dict(scene=(small, hs, large, hl), pixels=(A.data_large, A.data_small, plan), context=ctx)


def _used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def _growth(cycle):
    """Two warm-up cycles, six measured ones: min(last three readings) - reading after the warm-up, in bytes."""
    for _ in range(2):
        cycle()
    base = _used()
    readings = []
    for _ in range(6):
        cycle()
        readings.append(_used())
    growth = min(readings[-3:]) - base
    print("device memory in use after each cycle, MiB above the warm-up:",
          [round((r - base) / 2 ** 20, 2) for r in readings], "-> growth", round(growth / 2 ** 20, 2), "MiB")
    return growth


def _handle_cycle(inp):
    small, hs, large, hl = inp["scene"]
    h = _lib.CoregHandle(0)
    H.gpu_helio(h, small, hs, large, hl, LAGS, order=3)
    h.set_rotation("reference", ROT)
    h.set_rotation("small", ROT)
    H.gpu_carrington(h, small, hs, large, hl, LAGS, (32, 32))
    p_large, p_small, plan = inp["pixels"]
    h.pixels_set_large(p_large)
    h.pixels_set_small(p_small)
    assert h.pixels_sweep(plan).shape == (3, 3, 1)
    assert CC.gpu(h, inp["context"]).size == 9
    h.close()


def test_a_closed_handle_gives_its_device_memory_back(inputs):
    assert _growth(lambda: _handle_cycle(inputs)) < BOUND


def _multi_cycle(inp):
    small, hs, large, hl = inp["scene"]
    m = _lib.MultiHandle(n_devices=1)
    m.set_small(small)
    m.prepare_reference_helioprojective(large, hl, hs, 3)
    assert m.sweep_helioprojective(hs, hs, _lib.LagSet(*LAGS), order=3).shape == (9,)
    m.close()


def test_a_closed_multi_handle_gives_its_device_memory_back(inputs):
    assert _growth(lambda: _multi_cycle(inputs)) < BOUND


def test_closing_twice_unreferenced_or_with_a_sweep_in_flight(inputs):
    small, hs, large, hl = inputs["scene"]
    h = _lib.CoregHandle(0)
    before = H.gpu_helio(h, small, hs, large, hl, LAGS, order=3)
    assert np.isfinite(before).any()
    h.close()
    h.close()
    h = _lib.CoregHandle(0)
    h.close()
    del h
    gc.collect()
    # a device-output sweep still in flight when the handle goes: close() returns once the stream has drained ...
    h = _lib.CoregHandle(0)
    h.set_small(small)
    h.prepare_reference_helioprojective(large, hl, hs, 3)
    out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert h.sweep_helioprojective(hs, hs, _lib.LagSet(*LAGS), order=3, out_dev_ptr=out.data_ptr()) is None
    h.close()
    assert np.array_equal(out.cpu().numpy().reshape(before.shape), before, equal_nan=True)  # (... so the map is there)
    # ... and a fresh handle computes what the first one did
    with _lib.CoregHandle(0) as fresh:
        assert np.array_equal(H.gpu_helio(fresh, small, hs, large, hl, LAGS, order=3), before, equal_nan=True)
