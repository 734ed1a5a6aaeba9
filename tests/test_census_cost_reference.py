"""The census-transform matching cost of include/ws_stereo.h on the reference alone (no device): the NumPy restatement
equals the literal one, the closed forms of a constant image hold, a strictly increasing map of the grey levels changes
no census map while it changes the SAD map, and the inputs of the device tests do what they claim."""
import numpy as np
import pytest

from census_cost_inputs import grey3, inverted_pair, lut_pair, random_pair
from census_cost_inputs import periodic_pair, textured_pair
from census_cost_ref import BITS, search_np, search_py, slice_volume, transform_np, transform_py, volume, wta
from oracle import brute
from sgm_ref import sgm_from_volume

COSTS = ["census5x5", "census9x7"]
# (w, h): 1x1, 2x3, 3x9, 7x5 and 12x17 read as rows x columns, and as columns x rows
SIZES = [(1, 1), (3, 2), (9, 3), (5, 7), (17, 12), (2, 3), (3, 9), (7, 5), (12, 17)]


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_transform_numpy_equals_the_literal_witness(cost, w, h):
    L, _ = random_pair(w, h, 100 + w)
    got = transform_np(L, cost)
    want = np.array(transform_py(L, cost), dtype=np.uint64).reshape(h, w)
    assert got.dtype == np.uint64 and got.tobytes() == want.tobytes()
    assert int(got.max(initial=0)) < 1 << BITS[cost]
    # few grey levels: ties between neighbours and centre give 0 bits
    F = grey3(np.random.default_rng(w).integers(1, 4, size=(h, w)) * 60)
    assert transform_np(F, cost).tobytes() == np.array(transform_py(F, cost), dtype=np.uint64).reshape(h, w).tobytes()


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("w,h", SIZES)
def test_search_numpy_equals_the_literal_witness(cost, view, w, h):
    L, R = random_pair(w, h, 7 * w + h)
    L[h // 2, w // 2] = 0
    R[h // 2, w // 3] = 0
    for bs in (1, 3, 5):
        for mind, maxd in ((0, 6), (1, 40)):
            for sub in (False, True):
                got = search_np(L, R, view, bs, mind, maxd, cost, sub)
                want = search_py(L, R, view, bs, mind, maxd, cost, sub)
                assert got.tobytes() == want.tobytes(), (bs, mind, maxd, sub)


@pytest.mark.parametrize("cost", COSTS)
def test_search_witness_on_images_of_different_sizes(cost):
    L, R = random_pair(17, 12, 3, w2=13, h2=10)
    for view in ("left", "right"):
        for bs in (3, 5):
            assert search_np(L, R, view, bs, 0, 9, cost, True).tobytes() == search_py(L, R, view, bs, 0, 9, cost, True).tobytes()
    L, R = random_pair(13, 10, 4, w2=19, h2=10)
    for view in ("left", "right"):
        assert search_np(L, R, view, 3, 2, 11, cost).tobytes() == search_py(L, R, view, 3, 2, 11, cost).tobytes()


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", ["left", "right"])
def test_shortcuts_of_the_device_tests_equal_the_reference(cost, view):
    """slice_volume (one volume for every smaller max_disparity) and wta (the P1 = P2 = 0 map without walking paths)."""
    L, R = textured_pair(70, 23, 6, 9, w2=64, black=True)
    P, _ = periodic_pair(40, 9)
    for (A, B) in ((L, R), (P, P)):
        for bs, mind in ((1, 0), (5, 0), (7, 3)):
            big = volume(A, B, view, bs, mind, 5000, cost)
            for maxd in (1, 2, 9, 63, 64, 70, 5000):
                V = volume(A, B, view, bs, mind, maxd, cost)
                nd = V[0].shape[0]
                S = slice_volume(big, nd)
                assert all(np.array_equal(a, b) for a, b in zip(S, V)), (bs, mind, maxd)
                for sub in (False, True):
                    assert wta(V, view, sub).tobytes() == sgm_from_volume(V, view, 8, 0, 0, sub).tobytes(), (bs, mind, maxd, sub)


@pytest.mark.parametrize("cost", COSTS)
def test_constant_image(cost):
    """Every descriptor and every cost is 0, so the tie rule decides: a left-view interior pixel takes its largest
    candidate min(maxD, x - half), or the fallback x where it has none."""
    w, h, bs, D = 40, 20, 5, 16
    half = bs // 2
    img = np.full((h, w, 3), 90, np.uint8)
    assert not transform_np(img, cost).any()
    vol = volume(img, img, "left", bs, 0, D, cost)[0]
    assert (vol[vol >= 0] == 0).all()
    m = search_np(img, img, "left", bs, 0, D, cost)
    for x in range(half, w - half):
        d = min(D, x - half)
        assert (m[half:h - half, x] == (d if d else x)).all(), x
    assert not m[:half].any() and not m[:, :half].any()
    r = search_np(img, img, "right", bs, 2, D, cost)
    assert (r[:, :w - 2 - half] == 2).all()        # the smallest candidate


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", ["left", "right"])
def test_invariance_under_a_strictly_increasing_map(cost, view):
    L, R, lut = lut_pair(70, 21, 5, 11)
    base = search_np(L, R, view, 5, 0, 20, cost, True)
    assert transform_np(lut[R], cost).tobytes() == transform_np(R, cost).tobytes()
    assert search_np(L, lut[R], view, 5, 0, 20, cost, True).tobytes() == base.tobytes()
    assert search_np(lut[L], R, view, 5, 0, 20, cost, True).tobytes() == base.tobytes()
    sad = brute.block_left if view == "left" else brute.block_right
    assert (sad(L, R, 5, 0, 20, "sad") != sad(L, lut[R], 5, 0, 20, "sad")).any()


def test_inverted_pair_crosses_the_16_bit_bound_between_block_31_and_33():
    """What the device tests rely on: at 9x7 the inverted pair's window costs stay below 2^16 at block size 31 and pass it
    at 33, and an SGM map (P1 3, P2 20) changes when the costs are cut to 16 bits."""
    L, R = inverted_pair()
    v31 = volume(L, R, "left", 31, 0, 64, "census9x7")
    v33 = volume(L, R, "left", 33, 0, 64, "census9x7")
    assert 0 < v31[0].max() <= 62 * 31 * 31 < 65536
    assert 65535 < v33[0].max() <= 62 * 33 * 33
    want = sgm_from_volume(v33, "left", 8, 3, 20)
    cut = (np.where(v33[0] >= 0, v33[0] & 0xffff, -1),) + v33[1:]
    changed = int((sgm_from_volume(cut, "left", 8, 3, 20) != want).sum())
    print("max cost at 31:", int(v31[0].max()), "at 33:", int(v33[0].max()), "pixels changed by a 16-bit cut:", changed,
          "of", int(v33[2].sum()))
    assert changed > 0
