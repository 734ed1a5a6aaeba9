"""Pins tests/speckle_ref.py -- the statement of the speckle filter the device is compared with: the literal restatement of
OpenCV's wavefront loop and the connected-components witness agree bit for bit and count for count on every kind of map
the rules distinguish, and both give a hand-worked map.  No device, no library."""
import numpy as np
import pytest

from speckle_ref import (SPECIAL, checkerboard, filter_speckles, filter_speckles_wavefront, random_map, serpentine,
                         spiral)

F = np.float32
NAN, INF = np.nan, np.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def agree(a, new_val, max_size, max_diff):
    o1, c1 = filter_speckles_wavefront(a, new_val, max_size, max_diff)
    o2, c2 = filter_speckles(a, new_val, max_size, max_diff)
    assert np.array_equal(bits(o1), bits(o2)), (new_val, max_size, max_diff)
    assert c1 == c2, (c1, c2)
    return o2, c2


def test_hand_built_map():
    # new_val 0, max_speckle_size 2, max_diff 1:
    #   the 3s and the 4 form one region of 4 (kept); the lone 9 is one pixel (removed); the 7 / 8 pair is 2 (removed);
    #   the NaN joins nothing (removed); -0.0 is blank and stays -0.0; the 1 next to the 3 is 2 away (its own region:
    #   with the 1.5 below it, 2 pixels, removed); the +inf is alone (removed); the row of 5s is 4 (kept).
    a = np.array([[3, 3, 0, 9, -0.0, 7],
                  [3, 4, 0, 0, 0, 8],
                  [1, 0, NAN, 0, INF, 0],
                  [1.5, 0, 5, 5, 5, 5]], dtype=F)
    want = np.array([[3, 3, 0, 0, -0.0, 0],
                     [3, 4, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0],
                     [0, 0, 5, 5, 5, 5]], dtype=F)
    out, counts = agree(a, 0.0, 2, 1.0)
    assert np.array_equal(bits(out), bits(want))
    assert np.signbit(out[0, 4]) and not np.signbit(out[0, 3])
    assert counts == (1 + 2 + 1 + 2 + 1, 5)
    # max_diff 2 joins the 1 column to the 3s: one region of 6, and the 7 / 8 / 9 stay apart from each other (blank gaps)
    out, counts = agree(a, 0.0, 2, 2.0)
    assert out[2, 0] == 1 and out[3, 0] == 1.5 and out[0, 0] == 3
    assert counts == (1 + 2 + 1 + 1, 4)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (40, 1), (7, 9), (33, 65), (64, 70)])
def test_random_and_tie_heavy_maps(seed, shape):
    rng = np.random.default_rng(100 * seed + shape[0] * 7 + shape[1])
    levels = 3 if seed % 2 else 12
    a = random_map(rng, *shape, levels=levels, special=0.1 * (seed % 3), scale=0.5 if seed >= 4 else 1.0)
    for new_val, max_size, max_diff in ((0.0, 1, 0.0), (0.0, 5, 1.0), (-0.0, 20, 0.5), (2.0, 3, 1.25), (1.0, 10**9, INF),
                                        (0.0, 0, 1.0), (-1.0, 7, 2.0)):
        agree(a, new_val, max_size, max_diff)


@pytest.mark.parametrize("new_val", [0.0, -0.0, 2.5, -INF, INF, 1e30])
def test_every_special_value(new_val):
    rng = np.random.default_rng(7)
    a = rng.choice(SPECIAL, size=(24, 31)).astype(F)
    for max_size, max_diff in ((1, 0.0), (3, 1.0), (50, INF), (0, INF), (10**6, 0.5)):
        out, _ = agree(a, new_val, max_size, max_diff)
        blank = a == F(new_val)
        assert np.array_equal(bits(out)[blank], bits(a)[blank])  # blank pixels keep their bits


def test_infinities_join_only_finite_values_under_an_infinite_max_diff():
    a = np.array([[INF, 5, INF, INF, -INF, 1e30]], dtype=F)
    out, counts = agree(a, 0.0, 1, 1e38)
    assert counts == (6, 6)  # +-inf joins nothing under a finite max_diff, so all six are singletons
    out, counts = agree(a, 0.0, 3, INF)
    # inf - 5 = inf <= inf: the first three join through the 5; inf - inf is NaN: the second pair does not join;
    # -inf - inf = -inf, fabs = inf: the inf at x=3 joins the -inf, which joins 1e30 -- a region of 3 as well
    assert counts == (6, 2)


def test_nan_pixels_are_singletons():
    a = np.full((3, 4), NAN, dtype=F)
    out, counts = agree(a, 0.0, 1, INF)
    assert counts == (12, 12) and not out.any()
    out, counts = agree(a, 0.0, 0, INF)
    assert counts == (0, 0) and np.isnan(out).all()


@pytest.mark.parametrize("max_size", [0, 1, 100, 10**9])
def test_max_speckle_size_limits(max_size):
    a = random_map(np.random.default_rng(3), 30, 30, levels=4)
    out, counts = agree(a, 0.0, max_size, 0.0)
    if max_size == 0:
        assert counts == (0, 0) and np.array_equal(bits(out), bits(a))
    if max_size == 10**9:
        assert (out == 0).all() and counts[0] == int(np.count_nonzero(a != 0))  # every region goes


@pytest.mark.parametrize("shape", [(1, 97), (97, 1), (2, 70), (70, 2)])
def test_one_pixel_wide_maps(shape):
    a = random_map(np.random.default_rng(shape[0] * 3 + shape[1]), *shape, levels=3)
    for max_size in (0, 1, 2, 5, 1000):
        for max_diff in (0.0, 1.0, INF):
            agree(a, 0.0, max_size, max_diff)


@pytest.mark.parametrize("make", [serpentine, spiral])
@pytest.mark.parametrize("shape", [(5, 5), (33, 65), (70, 130)])
def test_serpentine_and_spiral_are_one_region(make, shape):
    a = make(*shape)
    n = int(np.count_nonzero(a))
    out, counts = agree(a, 0.0, n, 1.0)
    assert counts == (n, 1) and not out.any()
    out, counts = agree(a, 0.0, n - 1, 1.0)
    assert counts == (0, 0) and np.array_equal(bits(out), bits(a))


def test_serpentine_segments():
    a = serpentine(33, 70, segment=50)
    out, counts = agree(a, 0.0, 49, 1.0)
    assert counts[0] == int(np.count_nonzero(out != a)) and counts[1] == 1  # only the short last segment
    out, counts = agree(a, 0.0, 50, 1.0)
    assert counts[1] == int(np.ceil(np.count_nonzero(a) / 50))


def test_checkerboard_of_singletons():
    a = checkerboard(31, 47)
    n = int(np.count_nonzero(a))
    out, counts = agree(a, 0.0, 1, INF)
    assert counts == (n, n) and not out.any()
    out, counts = agree(a, 0.0, 0, INF)
    assert counts == (0, 0)


@pytest.mark.parametrize("bad", [dict(new_val=NAN), dict(max_diff=NAN), dict(max_diff=-1.0), dict(max_speckle_size=-1)])
def test_refusals(bad):
    kw = dict(new_val=0.0, max_speckle_size=10, max_diff=1.0)
    kw.update(bad)
    for f in (filter_speckles, filter_speckles_wavefront):
        with pytest.raises(ValueError):
            f(np.ones((2, 2), F), **kw)
    with pytest.raises(ValueError):
        filter_speckles(np.ones((0, 3), F))
