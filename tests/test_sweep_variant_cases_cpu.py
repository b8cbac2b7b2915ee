"""
The case table of tests/sweep_variant_cases.py against the instantiation list of csrc/sweep_variant.hpp, on the host:
tests/native/sweep_variant_pick.cpp prints the 71 entries and the index pick_sweep_variant gives every row of the table
and every forced pitch of tests/test_gpu_pitch.py::FAMILIES.  The indices reached are 0 ... 70, complete; each row's
predicted entry has the fields the row claims; the rows reach exactly the generic entries, one row each, and the forced
pitches exactly the pitched ones.  A row taken out of the table, or an entry added to make_sweep_variants() without a row,
fails here; the GPU tests (tests/test_gpu_sweep_variants.py, tests/test_gpu_pitch.py) take their expected index from the
same prediction.
"""
import collections

import pytest

from tests import sweep_variant_cases as V
from tests import test_gpu_pitch as P

pytestmark = pytest.mark.skipif(not V.have_compiler(), reason="no host C++ compiler")


def pitch_inputs():
    """(mode, order, f32, residus, pitch) of every forced pitch of test_gpu_pitch.py, with the pitch the family expects."""
    out = []
    for frame, order, f32_exact, pitches in P.FAMILIES:
        for p in pitches:
            out.append(((P.MODE_OF_FRAME[frame], order, int(f32_exact), 0, p), P.expected_pitch(order, f32_exact, p)))
    return out


def test_every_instantiation_is_some_rows_prediction():
    forced = pitch_inputs()
    entries, picks = V.native_picks([V.pick_input(r) for r in V.ROWS] + [i for i, _ in forced])
    assert len(entries) == 71 and len(set(entries)) == 71
    row_picks, pitch_picks = picks[:len(V.ROWS)], picks[len(V.ROWS):]
    assert min(picks) >= 0, "a pick outside the instantiation list"
    missing = sorted(set(range(len(entries))) - set(picks))
    assert not missing, f"entries no row and no forced pitch predicts: {[(i, entries[i]) for i in missing]}"
    assert sorted(set(picks)) == list(range(71))
    print(f"\n[sweep variants] {len(set(picks))} of {len(entries)} indices reached: {len(set(row_picks))} by the "
          f"{len(V.ROWS)} rows, {len(set(pitch_picks) - set(row_picks))} more by the {len(forced)} forced pitches")
    # each row's predicted entry is the one it claims, and agrees with the GPU tests' table of predictions
    for row, at in zip(V.ROWS, row_picks):
        assert entries[at] == V.claimed_variant(row), (V.row_id(row), at, entries[at])
        assert V.predicted()[V.row_id(row)] == at
    # the rows: exactly the generic entries; a compiled order has one row, a run-time-order kernel one per order
    generic = {i for i, e in enumerate(entries) if e[5] == 0}
    assert set(row_picks) == generic and len(generic) == 56
    per_entry = collections.Counter(row_picks)
    for i in generic:
        mode, order = entries[i][0], entries[i][1]
        n_orders = len(next(rt for m, _, rt, _ in V.FRAMES.values() if m == mode)) if order == V.ORDER_RT else 1
        assert per_entry[i] == n_orders >= 1 and (order != V.ORDER_RT or n_orders >= 2), (i, entries[i], per_entry[i])
    assert len({V.row_id(r) for r in V.ROWS}) == len(V.ROWS)
    # the forced pitches: the pitched entries, all 15, and the generic pitch-0 entry where the list holds no such pitch
    pitched = {i for i, e in enumerate(entries) if e[5] > 0}
    assert {at for at in pitch_picks if entries[at][5] > 0} == pitched and len(pitched) == 15
    for (inp, want_pitch), at in zip(forced, pitch_picks):
        mode, order, f32, _, p = inp
        assert entries[at] == (mode, order, bool(f32), mode != V.TRANSLATE, False, want_pitch), (inp, entries[at])
    dropped = [inp for (inp, want), _ in zip(forced, pitch_picks) if want == 0]
    assert dropped == [(V.TRANSLATE, 2, 0, 0, 185)]  # float64 pitch 185: deliberately not instantiated


def test_clean_path_rule_of_the_table():
    """has_clean_path restates kernels_sweep.hpp kCleanPath over the generic entries: 2 pixel types x 3 orders on the
    Carrington frame (no rounding), float32 only x 3 orders on the two homography modes."""
    entries, _ = V.native_picks([])
    clean = [e for e in entries if e[5] == 0 and V.has_clean_path(e)]
    assert len(clean) == 6 + 3 + 3
    assert all(e[0] != V.CAR and not e[4] and e[1] != V.ORDER_RT for e in clean)
    assert sum(1 for e in clean if not e[2]) == 3 and all(e[0] == V.TRANSLATE for e in clean if not e[2])
