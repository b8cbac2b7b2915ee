"""
Every compile-time LDS window pitch of k_sweep (csrc/sweep_variant.hpp: the 15 pitched entries of the instantiation list),
forced with the option "pitch" at small shapes, against the same call with the per-visit pitch ("pitch" 0).

The pitch moves the LDS addresses of the staged window only: neither the arithmetic nor the summation order depends on
it, so the maps are required to be EQUAL, NaN pattern included; each case prints its maximum difference before it asserts.

Shapes: image to align 64 x 56 px, so a staged window (image + apron) is at most 69 px wide and 61 rows high -- within the
smallest pitch (89) and, at 217 x 61 = 13 237 elements, within the 20 352-element LDS at the largest; every (tile, lag
batch) visit must therefore take the LDS path at every forced pitch (last_visit_counts).

pick_sweep_variant DROPS a pitch the list does not hold and runs the generic kernel, whose map is the same: equality
alone would not notice an ignored option or a pitched entry gone from the table.  Every sweep therefore also reports the
instantiation it ran (last_sweep_variant): the forced pitch where the family's list holds it, 0 for float64 pitch 185
(deliberately not instantiated), and the family's mode, order and pixel type.
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

LAGS = (17.0 + 8.0 * (np.arange(5) - 2), -9.0 + 8.0 * (np.arange(5) - 2), None, None, None)  # 5 x 5, +-1 px

# (frame, order, float32-exact pixels, forced pitches)
FAMILIES = [
    ("carrington", 2, True, (89, 121, 153, 185, 217)),
    ("carrington", 2, False, (89, 121, 153, 185)),  # float64 pixels: 185 is not instantiated and runs as pitch 0
    ("carrington", 3, True, (89, 121, 153)),
    ("helio-serial", 2, True, (89, 121)),
    ("helio-parallel", 2, True, (89, 121)),
]
# (csrc/sweep_variant.hpp) the mode each frame's sweep runs at these shapes: the full-grid semantics map the image onto the
# reference's wide field of view, where the host cannot prove the series inverse (eps_max >= 4e-6) -- exact division,
# kHomography = 1; the sub-map semantics stay within the image's own field -- kHomographySeries = 2; kTranslate = 0
MODE_OF_FRAME = {"carrington": 0, "helio-serial": 1, "helio-parallel": 2}
# the pitches the instantiation list holds (sweep_variant.hpp make_sweep_variants), by (order, float32 pixels)
COMPILED_PITCHES = {(2, True): (89, 121, 153, 185, 217), (2, False): (89, 121, 153), (3, True): (89, 121, 153)}


def expected_pitch(order, f32_exact, forced):
    """The pitch of the instantiation a forced pitch must run: itself where the list holds it, else 0 (dropped)."""
    return forced if forced in COMPILED_PITCHES[(order, f32_exact)] else 0


@pytest.mark.parametrize("frame,order,f32_exact,pitches", FAMILIES,
                         ids=[f"{f}-o{o}-{'f32' if e else 'f64'}" for f, o, e, _ in FAMILIES])
def test_forced_compile_time_pitch_equals_the_per_visit_pitch(gpu_handle, frame, order, f32_exact, pitches):
    small, hs, large, hl, _ = H.scene(small_shape=(56, 64), large_n=96, float32_exact=f32_exact)

    def sweep(prepare):
        if frame == "carrington":
            out = H.gpu_carrington(gpu_handle, small, hs, large, hl, LAGS, (72, 64), order=order, prepare=prepare)
        else:
            out = H.gpu_helio(gpu_handle, small, hs, large, hl, LAGS, order=order, prepare=prepare,
                              serial_semantics=frame == "helio-serial")
        st, vc = gpu_handle.last_stats(), gpu_handle.last_visit_counts()
        assert st["small_is_f32"] == int(f32_exact) and st["used_lds"] == 1
        assert vc["visits"] > 0 and vc["lds"] == vc["visits"], vc
        return out, gpu_handle.last_sweep_variant()

    def assert_variant(v, pitch):
        want = dict(mode=MODE_OF_FRAME[frame], order=order, f32=f32_exact, round=frame != "carrington", resid=False,
                    pitch=pitch)
        assert v["index"] >= 0 and {k: v[k] for k in want} == want, (v, want)

    try:
        gpu_handle.set_option("pitch", 0)
        want, v0 = sweep(True)
        assert np.isfinite(want).any()
        assert_variant(v0, 0)
        for p in pitches:
            gpu_handle.set_option("pitch", p)
            got, v = sweep(False)
            assert_variant(v, expected_pitch(order, f32_exact, p))
            assert (v["index"] == v0["index"]) == (v["pitch"] == 0)
            d = np.nanmax(np.abs(got - want))
            print(f"{frame} order={order} f32={f32_exact} pitch={p}: max|d| = {d:.3e}")
            assert np.array_equal(got, want, equal_nan=True), (p, d)
    finally:
        gpu_handle.set_option("pitch", -1)
