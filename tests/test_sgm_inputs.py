"""The staircase pairs of tests/sgm_inputs.py make the cross-register terms of the SGM path kernel decide winners: shown
here on the CPU reference alone, for every case tests/test_gpu_sgm_forms.py runs on the device.

The path kernel keeps disparity index j = 64 k + lane in register k, so the P1 link between j - 1 and j crosses
registers exactly where j % 64 == 0.  For each case the reference (tests/sgm_ref.py: sgm_np) runs once as it is and
once with that link left out at EVERY multiple of 64 (its `cut` argument: what a kernel whose lane 0 / lane 63 read
the wrong register would compute, up to the value it reads instead).  Then, for every multiple of 64 below nd, at
least one pixel whose map value changed has its true winner within 3 of that multiple: a device map equal to the
reference bit for bit has used each of those links.  The winners also reach the top live register, k = (nd - 1) // 64
(at the last nd of a band, 256 / 512 / 1024 / 2048, that is register NJ - 1)."""
import numpy as np
import pytest

from sgm_inputs import STAIRCASES, nj_of, staircase_case, staircase_disparity
from sgm_ref import sgm_from_volume, sgm_np, volume


@pytest.mark.parametrize("name", sorted(STAIRCASES))
def test_every_register_crossing_decides_a_winner(name):
    L, R, args, nd, _ = staircase_case(name)
    view, mind = args[0], args[2]
    d0 = 1 if view == "left" else mind
    cuts = list(range(64, nd, 64))
    assert cuts, "a case of one register has no crossing to show"
    view, bs, mind, maxd, cost, paths, p1, p2 = args
    V = volume(L, R, view, bs, mind, maxd, cost)
    assert V[0].shape[0] == nd
    node = V[2]
    ref = sgm_from_volume(V, view, paths, p1, p2, subpixel=True)
    cut = sgm_from_volume(V, view, paths, p1, p2, subpixel=True, cut=cuts)
    changed = (ref != cut) & node
    j = np.round(ref).astype(np.int64) - d0      # (the parabola moves a winner by less than half a step)
    near = {c: int((changed & (np.abs(j - c) <= 3)).sum()) for c in cuts}
    print(name, L.shape, "nd", nd, "changed", int(changed.sum()), "near each cut", near)
    assert all(near.values()), (name, [c for c in cuts if not near[c]])
    top = 64 * ((nd - 1) // 64)
    if nd in (256, 512, 1024, 2048):
        assert top == 64 * (nj_of(nd) - 1)
    assert (node & (j >= top)).any(), (name, top)


def test_the_staircase_steps_by_at_most_one_per_column():
    for view in ("left", "right"):
        d = staircase_disparity(700, 6, 1, 600, view)
        assert np.abs(np.diff(d, axis=1)).max() == 1 and d.min() == 1 and d.max() == 600
        assert set(np.unique(np.diff(d[:, 300:310], axis=0))) <= {1, -2}


def test_cut_argument_defaults_to_the_rule():
    L, R, args, nd, _ = staircase_case("129-left")
    assert np.array_equal(sgm_np(L, R, *args), sgm_np(L, R, *args, cut=None))
    assert np.array_equal(sgm_np(L, R, *args), sgm_np(L, R, *args, cut=[]))
