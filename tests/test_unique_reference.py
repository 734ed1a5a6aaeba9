"""The two restatements of the uniqueness ratio and confidence rules (tests/unique_ref.py) against each other and against
the SGM reference, without a device: they agree on seeded tiny pairs; the identities of the rules hold; a passing node
keeps sgm_np's value; the counts are the fail set's; and what the filter buys on teddy_quarter is pinned."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import brute
from sgm_ref import sgm_from_volume, sgm_np
from test_sgm_reference import TEDDY_QUARTER, tiny_case
from unique_ref import sums, unique_from_sums, unique_np, unique_py, volume

RATIOS = (0, 7, 15, 40, 100)


def case(seed):
    """tiny_case with every third seed on a census cost; sgm as the seed's (paths, p1, p2), sub-pixel on half of them."""
    L, R, view, bs, mind, maxd, cost, paths, p1, p2, _ = tiny_case(seed)
    if seed % 3 == 2:
        cost = ("census5x5", "census9x7")[(seed // 3) % 2]
        p1, p2 = p1 % 7, p1 % 7 + p2 % 40
    return L, R, view, bs, mind, maxd, cost, (paths, p1, p2), seed % 2 == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


@pytest.mark.parametrize("seed", range(36))
def test_the_two_restatements_agree(seed):
    L, R, view, bs, mind, maxd, cost, sgm, sub = case(seed)
    V = volume(L, R, view, bs, mind, maxd, cost)
    for s in (sgm, None):
        S = sums(V, s)
        for ratio in RATIOS:
            a = unique_from_sums(V, S, view, ratio, sub)
            m, c, counts = unique_py(V, S, view, ratio, sub)
            assert a["map"].tobytes() == m.tobytes(), (seed, s, ratio, np.argwhere(a["map"] != m)[:5].tolist())
            assert a["conf"].tobytes() == c.tobytes(), (seed, s, ratio, np.argwhere(a["conf"] != c)[:5].tolist())
            assert a["counts"] == counts, (seed, s, ratio)


def test_the_seeds_cover_the_rules():
    """Both views, SAD, SSD and both census costs, 4 and 8 paths, sub-pixel; failing, passing and uncontested nodes."""
    seen = set()
    fail = keep = lone = 0
    for seed in range(36):
        L, R, view, bs, mind, maxd, cost, sgm, sub = case(seed)
        seen |= {view, cost, sgm[0], ("sub", sub)}
        r = unique_np(L, R, view, bs, mind, maxd, cost, 15, sgm, sub)
        fail += int(r["fail"].sum())
        keep += int((r["contested"] & ~r["fail"]).sum())
        lone += r["counts"][1] - int(r["contested"].sum())
    assert seen >= {"left", "right", "sad", "ssd", "census5x5", "census9x7", 4, 8, ("sub", True), ("sub", False)}
    assert fail >= 20 and keep >= 100 and lone >= 100, (fail, keep, lone)


@pytest.mark.parametrize("seed", range(2, 26, 2))
def test_identities(seed):
    L, R, view, bs, mind, maxd, cost, sgm, sub = case(seed)
    V = volume(L, R, view, bs, mind, maxd, cost)
    S = sums(V, sgm)
    # (a) ratio 0 is the search's own map
    assert unique_from_sums(V, S, view, 0, sub)["map"].tobytes() == sgm_from_volume(V, view, *sgm, subpixel=sub).tobytes()
    assert unique_from_sums(V, sums(V), view, 0, sub)["map"].tobytes() == sgm_from_volume(V, view, 4, 0, 0, subpixel=sub).tobytes()
    # (b) S = C and S = paths * C: the same map, the same confidence
    for ratio in RATIOS:
        a = unique_from_sums(V, sums(V), view, ratio, sub)
        b = unique_from_sums(V, sums(V, (sgm[0], 0, 0)), view, ratio, sub)
        assert a["map"].tobytes() == b["map"].tobytes() and a["conf"].tobytes() == b["conf"].tobytes(), ratio
        assert a["counts"] == b["counts"]
    # (c) the fail set grows with ratio; the confidence does not depend on it
    prev = None
    for ratio in range(0, 101, 5):
        r = unique_from_sums(V, S, view, ratio, sub)
        if prev is not None:
            assert not (prev["fail"] & ~r["fail"]).any(), ratio
            assert prev["conf"].tobytes() == r["conf"].tobytes()
        else:
            assert not r["fail"].any()
        prev = r
    assert (prev["fail"] == (prev["contested"] & (prev["smin"] > 0))).all()   # ratio 100


@pytest.mark.parametrize("seed", range(12))
def test_rule_4_against_sgm_np_and_the_counts(seed):
    L, R, view, bs, mind, maxd, cost, sgm, sub = case(seed)
    if cost.startswith("census"):
        cost = "sad"
    base = sgm_np(L, R, view, bs, mind, maxd, cost, *sgm, subpixel=sub)
    r = unique_np(L, R, view, bs, mind, maxd, cost, 25, sgm, sub)
    assert (r["map"][r["fail"]] == 0).all()
    assert bits(r["map"][~r["fail"]]) == bits(base[~r["fail"]])
    V = volume(L, R, view, bs, mind, maxd, cost)
    node = V[2]
    assert r["counts"] == (int(r["fail"].sum()), int(node.sum()))
    assert not (r["fail"] & ~node).any() and not (r["contested"] & ~node).any()
    # the confidence: 0 outside the nodes, 1 exactly on the uncontested ones, in [0, 1] everywhere
    assert (r["conf"][~node] == 0).all() and (r["conf"][node & ~r["contested"]] == 1).all()
    assert (r["conf"] >= 0).all() and (r["conf"] <= 1).all()
    # at most two candidates, or three with the winner in the middle: uncontested
    count = (V[0] >= 0).sum(axis=0)
    first = (V[0] >= 0).argmax(axis=0)
    assert not (node & (count <= 2) & r["contested"]).any()
    assert not (node & (count == 3) & (r["jb"] == first + 1) & r["contested"]).any()
    assert (r["contested"] == (node & ((r["jb"] - first >= 2) | (first + count - 1 - r["jb"] >= 2)))).all()


def test_a_zero_tie_passes_at_every_ratio():
    """Two identical constant images: every cost is 0, so m2 == Smin == 0 at every contested node."""
    L = np.full((9, 30, 3), 80, np.uint8)
    for ratio in (1, 50, 100):
        for sgm in (None, (8, 0, 0)):
            r = unique_np(L, L.copy(), "left", 3, 0, 8, "sad", ratio, sgm)
            assert r["contested"].sum() > 50 and not r["fail"].any()
            assert (r["conf"][r["contested"]] == 0).all() and (r["m2"][r["contested"]] == 0).all()
        # with penalties the rivals of a zero-cost winner cost more than it: still no failure, and full confidence
        r = unique_np(L, L.copy(), "left", 3, 0, 8, "sad", ratio, (8, 3, 9))
        assert not r["fail"].any() and (r["conf"][r["contested"]] == 1).all()


# teddy_quarter, left view, D = 64, 8 paths, SAD: TEDDY_QUARTER's (block_size, P1, P2) and the ratio ->
# (evaldisp's bad % among the kept nodes, failed nodes, nodes), from the reference
TEDDY_UNIQUE = {
    (3, 216, 864, 10): (5.207542896270752, 12366, 166731),
    (3, 216, 864, 15): (4.173391342163086, 17900, 166731),
    (5, 600, 2400, 10): (5.8709869384765625, 12134, 165095),
    (5, 600, 2400, 15): (4.7883687019348145, 17618, 165095),
}


@pytest.mark.parametrize("key", sorted(TEDDY_QUARTER))
def test_teddy_quarter_kept_pixels_are_better(key):
    bs, p1, p2 = key
    g = load_golden("teddy_quarter")
    V = volume(g["left"], g["right"], "left", bs, 0, 64, "sad")
    S = sums(V, (8, p1, p2))
    bad0 = TEDDY_QUARTER[key][0]
    prev = bad0
    for ratio in (10, 15):
        r = unique_from_sums(V, S, "left", ratio)
        kept = np.where(r["fail"], 0, g["mask"])   # evaldisp on the kept pixels alone
        e = brute.evaldisp_np(r["map"], g["gt"], kept, 2.0, 64)
        got = (e["bad"], ) + r["counts"]
        assert got == TEDDY_UNIQUE[key + (ratio,)]
        assert e["bad"] < prev
        prev = e["bad"]
        # the dropped pixels are mostly wrong ones: more than half of them are bad in the unfiltered map
        base = unique_from_sums(V, S, "left", 0)["map"]
        dropped = np.where(r["fail"], g["mask"], 0)
        assert brute.evaldisp_np(base, g["gt"], dropped, 2.0, 64)["bad"] > 50.0
