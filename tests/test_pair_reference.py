"""The two restatements of "both views from one volume" (tests/pair_ref.py) against each other, without a device: they
agree on the tiny seeds of tests/test_sgm_reference.py in both views; sgm == NULL and zero penalties give the same maps;
the derived map is not the other view's searched map; and what the check gains from it on teddy_quarter is pinned."""
import numpy as np
import pytest

import lr_ref
from conftest import load_golden
from oracle import brute
from pair_ref import derived_np, derived_py, other_shape, pair_np
from test_sgm_reference import tiny_case
from unique_ref import sums, unique_from_sums, volume


def tiny_views(seed):
    """The seed as it is, and with the view flipped where the geometry allows (the right view takes a right image at
    most one row taller than the left one; tiny_case never draws one)."""
    L, R, view, bs, mind, maxd, cost, paths, p1, p2, sub = tiny_case(seed)
    yield L, R, view, bs, mind, maxd, cost, paths, p1, p2
    if R.shape[0] <= L.shape[0] + 1:
        flipped = "right" if view == "left" else "left"
        yield L, R, flipped, bs, 0 if flipped == "left" else mind, maxd, cost, paths, p1, p2


@pytest.mark.parametrize("seed", range(48))
def test_the_two_restatements_agree(seed):
    runs = 0
    for L, R, view, bs, mind, maxd, cost, paths, p1, p2 in tiny_views(seed):
        V = volume(L, R, view, bs, mind, maxd, cost)
        for sgm in ((paths, p1, p2), None):
            S = sums(V, sgm)
            a = derived_np(S, V[1], view, other_shape(L, R, view))
            b = derived_py(S, V[1], view, other_shape(L, R, view))
            assert a.shape == other_shape(L, R, view)
            assert a.tobytes() == b.tobytes(), (seed, view, sgm, np.argwhere(a != b)[:5].tolist())
            runs += 1
    assert runs == 4, "both views of every seed"


def test_the_tiny_seeds_meet_ties_and_empty_pixels():
    ties = empty = 0
    for seed in range(48):
        for L, R, view, bs, mind, maxd, cost, paths, p1, p2 in tiny_views(seed):
            V = volume(L, R, view, bs, mind, maxd, cost)
            S = sums(V, None)
            a = derived_np(S, V[1], view, other_shape(L, R, view))
            ties += int((a != derived_np(S, V[1], view, other_shape(L, R, view), tie="other")).sum())
            empty += int((a == 0).sum())
    assert ties > 50 and empty > 500, (ties, empty)


@pytest.mark.parametrize("seed", range(0, 48, 3))
def test_null_sgm_is_zero_penalties(seed):
    """Rule 7: S = paths * C."""
    for L, R, view, bs, mind, maxd, cost, paths, p1, p2 in tiny_views(seed):
        a = pair_np(L, R, view, bs, mind, maxd, cost, sgm=None, lr=(1.0, True))
        b = pair_np(L, R, view, bs, mind, maxd, cost, sgm=(paths, 0, 0), lr=(1.0, True))
        for k in ("left", "right", "checked_left", "checked_right"):
            assert a[k].tobytes() == b[k].tobytes(), (seed, view, k)
        assert a["lr_counts"] == b["lr_counts"]


def test_the_derived_map_is_not_the_searched_map():
    """The derived map's windows are the base view's: it differs from the direct search of the other view."""
    differ = pixels = 0
    for seed in range(48):
        L, R, view, bs, mind, maxd, cost, paths, p1, p2, _ = tiny_case(seed)
        if view != "left" or R.shape[0] > L.shape[0] + 1:
            continue
        res = pair_np(L, R, "left", bs, 0, maxd, cost, sgm=(paths, p1, p2))
        VR = volume(L, R, "right", bs, 0, maxd + 1, cost)   # the right view's range ends before max_disparity
        direct = unique_from_sums(VR, sums(VR, (paths, p1, p2)), "right", 0)["map"]
        differ += int((res["right"] != direct).sum())
        pixels += direct.size
    assert differ > pixels // 20, (differ, pixels)


# teddy_quarter, left base, 5 x 5 SAD, D = 64, max_diff 1, no fill: sgm -> (failure counts (left, right) of the derived
# route, of two searches, evaldisp bad-2.0 (bad %, invalid %) of the checked left map of the derived route, of two searches,
# bad % of the raw left map: tests/test_sgm_reference.py's figures)
TEDDY_QUARTER = {
    (8, 600, 2400): ((19066, 17030), (21599, 18596), (6.256738662719727, 5.287759304046631), (5.459036827087402, 6.0138115882873535),
                     8.381668090820312),
    None: ((43224, 41096), (51131, 49393), (9.307657241821289, 20.708173751831055), (8.17081356048584, 25.721616744995117),
           21.36598777770996),
}


@pytest.mark.parametrize("sgm", [(8, 600, 2400), None], ids=["sgm", "block"])
def test_teddy_quarter_checked_maps(sgm):
    g = load_golden("teddy_quarter")
    L, R = g["left"], g["right"]
    res = pair_np(L, R, "left", 5, 0, 64, "sad", sgm=sgm, lr=(1.0, False))
    VR = volume(L, R, "right", 5, 0, 64, "sad")
    right = unique_from_sums(VR, sums(VR, sgm), "right", 0)["map"]
    two_left, _, two_counts = lr_ref.lr_check(res["left"].astype(np.float32), right.astype(np.float32), 1.0, False)
    e = brute.evaldisp_np(res["checked_left"].astype(np.float64), g["gt"], g["mask"], 2.0, 64)
    e2 = brute.evaldisp_np(two_left.astype(np.float64), g["gt"], g["mask"], 2.0, 64)
    raw = brute.evaldisp_np(res["left"], g["gt"], g["mask"], 2.0, 64)
    assert (res["lr_counts"], two_counts, (e["bad"], e["invalid"]), (e2["bad"], e2["invalid"]), raw["bad"]) == TEDDY_QUARTER[sgm]
    assert e["bad"] < raw["bad"] and e2["bad"] < e["bad"], "the derived route keeps most of the check's gain, not all"
    assert raw["bad"] - e["bad"] > 0.6 * (raw["bad"] - e2["bad"])
