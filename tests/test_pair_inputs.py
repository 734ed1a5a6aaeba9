"""The inputs of tests/test_gpu_pair.py (tests/pair_inputs.py) bite, shown on the reference alone: the periodic pairs'
derived maps are decided by the tie rule, the staircases' derived winners fall in every 64-lane chunk of a curve, and
every class of derived pixel occurs -- none, one candidate, and a winner that comes from another span's base column."""
import numpy as np
import pytest

from pair_inputs import (PERIODIC, STAIRCASES, candidate_counts, case_sums, derived_of, kernel_constant, periodic_case,
                         staircase_case)
from pair_ref import other_shape


def test_the_kernel_constants_are_named():
    assert kernel_constant("kPairSpan") >= 64 and kernel_constant("kPairSwitchWidth") == kernel_constant("kPairSpan")


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("name", sorted(PERIODIC))
def test_periodic_pairs_are_decided_by_the_tie_rule(name, view):
    """With zero penalties the candidates of a derived pixel tie exactly; the other view's tie rule gives another map.
    (With penalties the ties all but vanish: the device tests use sgm None and (4, 0, 0) on these.)"""
    L, R, maxd = periodic_case(name)
    for sgm in (None, (4, 0, 0)):
        a = derived_of(L, R, view, 3, 0, maxd, "sad", sgm)
        b = derived_of(L, R, view, 3, 0, maxd, "sad", sgm, tie="other")
        assert int((a != b).sum()) >= 200, (name, view, sgm, int((a != b).sum()))


@pytest.mark.parametrize("name", sorted(STAIRCASES))
def test_staircase_winners_fall_in_every_chunk(name):
    L, R, (view, bs, mind, maxd, cost), sgm, nd = staircase_case(name)
    _, jb = derived_of(L, R, view, bs, mind, maxd, cost, sgm, winners=True)
    chunks = set((jb[jb >= 0] // 64).tolist())
    assert chunks == set(range((nd + 63) // 64)), (name, sorted(set(range((nd + 63) // 64)) - chunks))


def test_every_pixel_class_occurs():
    span = kernel_constant("kPairSpan")
    for name in ("1025-left", "1025-right"):
        L, R, (view, bs, mind, maxd, cost), sgm, nd = staircase_case(name)
        V, S = case_sums(L, R, view, bs, mind, maxd, cost, sgm)
        shape = other_shape(L, R, view)
        assert shape[1] > 2 * span
        n = candidate_counts(S, V[1], view, shape)
        out, jb = derived_of(L, R, view, bs, mind, maxd, cost, sgm, winners=True)
        assert (n == 0).sum() > 0 and (n == 1).sum() > 0 and (n > 64).sum() > 0, name
        assert ((n == 0) == (jb < 0)).all() and (out[n == 0] == 0).all()
        xs = np.broadcast_to(np.arange(shape[1])[None, :], shape)
        base_col = np.where(jb >= 0, xs + (jb + V[1]) * (1 if view == "left" else -1), xs)
        crossing = (jb >= 0) & (base_col // span != xs // span)
        assert crossing.sum() > 100, (name, int(crossing.sum()))
        assert ((jb >= 0) & (np.abs(base_col - xs) >= span)).any(), "a winner from beyond the neighbouring span"
