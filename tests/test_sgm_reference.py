"""The two restatements of the semi-global matching rules (tests/sgm_ref.py) against each other and against the block
search's references, without a device: they agree on seeded tiny pairs; at P1 = P2 = 0 the NumPy one is the block search
(the C oracle, and the fast reference's float32 sub-pixel maps); the quality it buys on teddy_quarter is pinned; and the
bound of the arithmetic holds at its extreme."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import brute
from sgm_inputs import GEOMETRIES, geometry_case
from sgm_ref import sgm_np, sgm_py
from test_subpixel_reference import shifted_pair


def tiny_case(seed):
    """A seeded tiny pair and its parameters: both views, 4 and 8 paths, SAD and SSD, black pixels, few-level images,
    right view with min_disparity > 0, unequal sizes, sub-pixel."""
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(7, 25)), int(rng.integers(5, 17))
    view = ("left", "right")[seed % 2]
    cost = ("sad", "ssd")[(seed // 2) % 2]
    paths = (4, 8)[(seed // 4) % 2]
    bs = int(rng.choice([1, 3, 5]))
    levels = 2 + seed % 3 if seed % 3 == 0 else None
    t = int(rng.integers(0, 4))
    L, R = shifted_pair(w, h, t, seed, noise=0 if levels else 6, levels=levels, block=2)
    if seed % 5 == 1:   # unequal sizes: a narrower, shorter right image (never taller: the reference would throw)
        R = R[: h - int(rng.integers(0, 3)), : w - int(rng.integers(1, 4))]
    L, R = L.copy(), R.copy()
    if seed % 4 == 2:   # black pixels inside the image
        L[h // 2, 1: w // 2] = 0
        R[h // 3, w // 3:] = 0
        L[1:3, w - 3] = 0
    mind = int(rng.integers(0, 3)) if view == "right" else 0
    maxd = mind + int(rng.integers(1, 13))
    p1 = int(rng.integers(0, 60))
    p2 = p1 + int(rng.integers(0, 400))
    return L, R, view, bs, mind, maxd, cost, paths, p1, p2, seed % 3 == 1


@pytest.mark.parametrize("seed", range(48))
def test_the_two_restatements_agree(seed):
    L, R, view, bs, mind, maxd, cost, paths, p1, p2, sub = tiny_case(seed)
    a = sgm_np(L, R, view, bs, mind, maxd, cost, paths, p1, p2, subpixel=sub)
    b = sgm_py(L, R, view, bs, mind, maxd, cost, paths, p1, p2, subpixel=sub)
    assert a.tobytes() == b.tobytes(), (seed, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_the_two_restatements_agree_on_a_larger_right_image(name):
    """A right image wider than the left one, taller, or both (the right view: wider by more than max_disparity, taller
    by the one row it may be): the geometries of tests/test_gpu_sgm_forms.py at a size the literal loops can walk."""
    maxd = 6
    L, R, view, mind = geometry_case(name, 15, 8, maxd)
    assert R.shape[1] > L.shape[1] or R.shape[0] > L.shape[0]
    for i, (bs, cost, paths, p1, p2, sub) in enumerate(((3, "sad", 8, 7, 90, True), (5, "ssd", 4, 40, 900, False))):
        a = sgm_np(L, R, view, bs, mind, maxd, cost, paths, p1, p2, subpixel=sub)
        b = sgm_py(L, R, view, bs, mind, maxd, cost, paths, p1, p2, subpixel=sub)
        assert a.shape == R.shape[:2] if view == "right" else a.shape == L.shape[:2]
        assert a.tobytes() == b.tobytes(), (name, i, np.argwhere(a != b)[:5].tolist())
        if view == "right" and R.shape[1] > L.shape[1] + maxd:   # the columns without a candidate hold -x
            xs = np.arange(L.shape[1], R.shape[1])
            rows = min(L.shape[0], R.shape[0])
            assert (a[:rows, L.shape[1]:] == -xs[None, :]).all()


def test_the_restatements_are_not_the_block_search():
    """Nonzero penalties change maps: the agreement above is not an agreement on block-search maps."""
    changed = 0
    for seed in range(48):
        L, R, view, bs, mind, maxd, cost, paths, p1, p2, sub = tiny_case(seed)
        base = sgm_np(L, R, view, bs, mind, maxd, cost, paths, 0, 0, subpixel=sub)
        changed += not np.array_equal(base, sgm_np(L, R, view, bs, mind, maxd, cost, paths, 50, 2000, subpixel=sub))
    assert changed >= 10


@pytest.mark.parametrize("seed", range(24))
def test_zero_penalties_are_the_block_search(oracle, seed):
    L, R, view, bs, mind, maxd, cost, paths, _, _, _ = tiny_case(seed)
    if view == "left" and bs % 2 == 0:
        pytest.fail("tiny_case draws odd block sizes")
    block = (oracle.block_left if view == "left" else oracle.block_right)(L, R, bs, mind, maxd, cost=cost)
    assert sgm_np(L, R, view, bs, mind, maxd, cost, paths, 0, 0).tobytes() == block.tobytes()
    fast = (oracle.fast_left if view == "left" else oracle.fast_right)(L, R, bs, mind, maxd, cost=cost, subpixel="float32")
    assert sgm_np(L, R, view, bs, mind, maxd, cost, paths, 0, 0, subpixel=True).tobytes() == fast.tobytes()


@pytest.mark.parametrize("view,mind", [("left", 0), ("right", 0), ("right", 3)])
def test_zero_penalties_at_a_larger_size(oracle, view, mind):
    L, R = shifted_pair(96, 40, 9, 21)
    for cost, bs in (("ssd", 7), ("sad", 5)):
        fast = (oracle.fast_left if view == "left" else oracle.fast_right)(L, R, bs, mind, 32, cost=cost, subpixel="float32")
        assert sgm_np(L, R, view, bs, mind, 32, cost, 8, 0, 0, subpixel=True).tobytes() == fast.tobytes()
        ref = (brute.block_left if view == "left" else brute.block_right)(L, R, bs, mind, 32, cost)
        assert sgm_np(L, R, view, bs, mind, 32, cost, 4, 0, 0).tobytes() == ref.tobytes()


# evaldisp on teddy_quarter, left view, D = 64, 8 paths, SAD: (block_size, P1, P2) -> (SGM bad %, block search bad %)
TEDDY_QUARTER = {(5, 600, 2400): (8.381668090820312, 21.36598777770996), (3, 216, 864): (7.631051063537598, 31.400379180908203)}


@pytest.mark.parametrize("key", sorted(TEDDY_QUARTER))
def test_teddy_quarter_bad_pixels_fall(key):
    bs, p1, p2 = key
    g = load_golden("teddy_quarter")
    sgm = sgm_np(g["left"], g["right"], "left", bs, 0, 64, "sad", 8, p1, p2)
    block = brute.block_left(g["left"], g["right"], bs, 0, 64, "sad")
    e = brute.evaldisp_np(sgm, g["gt"], g["mask"], 2.0, 64)
    eb = brute.evaldisp_np(block, g["gt"], g["mask"], 2.0, 64)
    assert (e["bad"], eb["bad"]) == TEDDY_QUARTER[key]
    assert e["bad"] < eb["bad"] / 2


def extreme_pair(w=80, h=70):
    L = np.full((h, w, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    R = np.repeat(np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
    return L, R


def test_extreme_bound():
    """block_size 63, SSD, a 0/255 checkerboard, P2 = 2^31 - 1: C < 2^30, every Lr < 2^32, S needs more than 32 bits."""
    L, R = extreme_pair()
    big = 2 ** 31 - 1
    cmax = 3 * 255 * 255 * 63 * 63
    assert cmax < 2 ** 30
    for view, p1 in (("left", big), ("left", 0), ("right", 1000)):
        m, lmax = sgm_np(L, R, view, 63, 0, 16, "ssd", 8, p1, big, return_lmax=True)
        assert lmax < 2 ** 32, (view, p1, lmax)
        if p1 == big:   # a candidate its predecessor lacks pays P1 or P2: the largest Lr passes 2^31, eight of them 2^32
            assert lmax > 2 ** 31 and 8 * lmax > 2 ** 32, lmax
        assert np.isfinite(m).all()
