"""What tests/test_gpu_persistent_nonfinite.py takes for granted before its first GPU call, held without a GPU: the
preconditions on the staged windows (every NaN / infinite pixel column certainly staged by the tiles of its tile column
and certainly not by any other tile; which helioprojective tiles are interior) and what the CPU oracles say about its
images (no poisoned term, `finite_terms` equal to `count`, counts that differ between lags, the poisoned reference).
The functions are that module's own, cached: the GPU tests call the same ones."""
import numpy as np
import pytest

from tests import test_gpu_persistent_nonfinite as T


@pytest.mark.parametrize("order", [1, 2, 3])
def test_carrington_precondition(order):
    x0, x1, y0, y1 = T.carrington_precondition(order)
    print(f"\n[persistent cpu] order {order}: samples span x {x0:.1f} ... {x1:.1f}, y {y0:.1f} ... {y1:.1f}; columns {T.X}")
    xlo, xhi, _, _ = T.carrington_boxes()
    win = T.windows(xlo, xhi, T.APRON[order])
    for c in range(4):
        own = [x for x in range(T.W) if T.certainly_staged(x, win)[:, c].all()
               and all(T.certainly_not_staged(x, win)[:, t].all() for t in range(4) if t != c)]
        print(f"[persistent cpu] order {order}: pixel columns under tile column {c} alone: {own}")
        assert T.X[c] in own and len(own) >= 4


@pytest.mark.parametrize("name", ["P", "P'", "Q", "Q'"])
def test_carrington_oracle_counts(name):
    n = T.oracle_counts(name, True)
    print(f"\n[persistent cpu] {name}: counts {n.min():.0f} ... {n.max():.0f} of 65536, {np.unique(n).size} different")
    assert n.shape == (17, 17, 1, 1, 1, 1) and np.unique(n).size > 1


def test_poisoned_reference():
    ref, m = T.poisoned_case("Q", True)
    print(f"\n[persistent cpu] poisoned terms a lag: {m['poisoned'].min():.0f} ... {m['poisoned'].max():.0f}; "
          f"lags with a number: {np.isfinite(m['masked']).sum()} of {m['masked'].size}")
    assert (ref <= 0).sum() == 4


def test_helioprojective_precondition_and_counts():
    assert T.helio_precondition()
    for name in ("H", "H'"):
        _, want, n = T.helio_case(name)
        print(f"\n[persistent cpu] helioprojective {name}: counts {n.min():.0f} ... {n.max():.0f}")
        assert want.shape[:2] == (13, 12)


def test_border_case():
    *_, want, n = T.border_case()
    print(f"\n[persistent cpu] bounded: counts {np.nanmin(n):.0f} ... {np.nanmax(n):.0f}, "
          f"{np.isfinite(want).sum()} of {want.size} lags with a coefficient")
