"""The pairs of tests/mfma_inputs.py do what tests/test_gpu_mfma_census.py relies on -- shown on the CPU reference
(oracle.fast_left, 7 x 7 SSD) alone, no device:

  * disparity_ladder with ds = 1 .. 256: every band's clean rows equal d from column d + 3 on, and every cell
    (d, (x - 3) % 128) -- every live accumulator register of every lane of every wave of the matrix kernel -- is a
    winner somewhere: 32768 of 32768 cells;
  * tie_ladder: on a band's clean rows the map is p * (min(D, x - 3) // p), the largest tying candidate;
  * the pair of the range sweep (range_sweep_pair) has winners on both sides of every step of the kernel's per-wave
    `active` mask.
"""
import numpy as np
import pytest

import mfma_inputs as mi


def _left(oracle, left, right, maxd):
    return oracle.fast_left(left, right, mi.BS, 0, maxd, cost="ssd")


@pytest.mark.parametrize("shape", [(700, 9), (520, 8)], ids=["700x9", "520x8"])
def test_ladder_census_is_complete(oracle, shape):
    w, band = shape
    ds = list(range(1, 257))
    left, right = mi.disparity_ladder(w, band, 11, ds)
    assert left.shape == (band * 256, w, 3) and left.min() >= 1 and right.min() >= 1
    m = _left(oracle, left, right, 256)
    for y, x0, d in mi.ladder_expected(w, band, ds, 256):
        assert (m[y, x0:w - mi.HALF] == d).all(), (y, d, np.flatnonzero(m[y, x0:w - mi.HALF] != d)[:5] + x0)
    assert len(mi.ladder_expected(w, band, ds, 256)) == 256 * (band - 6)
    cells = mi.census(m)
    missing = np.argwhere(~cells)
    assert cells.shape == (256, 128) and int(cells.sum()) == 32768, \
        [(int(d) + 1, int(c), mi.slot_of(int(d) + 1, int(c) + mi.HALF)) for d, c in missing[:5]]


def test_slots_are_one_register_each():
    """slot_of is a bijection between (d, tile column) and the registers whose candidate is inside the range."""
    seen = set()
    for d in range(1, 257):
        for c in range(128):
            t, i, h, n, wx, wv = mi.slot_of(d, c + mi.HALF)
            assert 0 <= t <= 8 and 0 <= i < 16 and h in (0, 1) and n == c % 32 and wx == c // 32 and wv == (t >= 5)
            m = (i & 3) + 8 * (i >> 2) + 4 * h
            assert 32 * (8 - t) + n - m == d - 1
            seen.add((t, i, h, n, wx))
    assert len(seen) == 32768


@pytest.mark.parametrize("maxd", [100, 255])
def test_ladder_under_a_shorter_range(oracle, maxd):
    """The ladder's bands up to D keep their winner; the bands beyond hold noise, where any candidate may win."""
    w, band, ds = 520, 8, list(range(1, 257))
    left, right = mi.disparity_ladder(w, band, 11, ds)
    m = _left(oracle, left, right, maxd)
    exp = mi.ladder_expected(w, band, ds, maxd)
    assert len(exp) == maxd * (band - 6)
    for y, x0, d in exp:
        assert (m[y, x0:w - mi.HALF] == d).all(), (y, d)
    assert int(mi.census(m, maxd).sum()) == 128 * maxd


@pytest.mark.parametrize("band", [9, 12])
def test_tie_ladder_largest_tying_candidate_wins(oracle, band):
    w, maxd = 640, 256
    left, right = mi.tie_ladder(w, band, mi.TIE_PERIODS, 5)
    assert left.shape == (band * len(mi.TIE_PERIODS), w, 3) and np.array_equal(left, right) and left.min() >= 1
    m = _left(oracle, left, right, maxd)
    for k, p in enumerate(mi.TIE_PERIODS):
        x0, want = mi.tie_expected_row(w, p, maxd)
        for y in mi.clean_rows(band, k):
            assert np.array_equal(m[y, x0:w - mi.HALF], want), (p, y, np.flatnonzero(m[y, x0:w - mi.HALF] != want)[:5] + x0)
    # period 1: every candidate wins in turn; 160: the only multiple inside the range, a lone winner beside a tile boundary
    x0, want = mi.tie_expected_row(w, 1, maxd)
    assert set(want.tolist()) == set(float(d) for d in range(1, 257))
    assert set(mi.tie_expected_row(w, 160, maxd)[1].tolist()) == {160.0}
    if band == 12:                                                 # tall enough for the matrix kernel's selection rule
        assert band * len(mi.TIE_PERIODS) - 2 * mi.HALF >= 192


def test_range_sweep_pair_has_winners_around_every_step(oracle):
    """At max_disparity = 32 k + 1 and 32 k + 2 (dcount = D: the step of the `active` mask is at dcount = 32 k + 2,
    where tile 8 - k - 1 gets its first live candidate, e = 32 k + 1 = n - m + 32 (k + 1), held by lane column n = 0 in
    row m = 31 alone) the candidate d = D wins somewhere, and so does d = 1."""
    w, h = 390, 198
    left, right = mi.range_sweep_pair(w, h)
    for k in range(8):
        for maxd in (32 * k + 1, 32 * k + 2, 32 * k + 3):
            m = _left(oracle, left, right, maxd)[mi.HALF:h - mi.HALF, mi.HALF:w - mi.HALF]
            assert (m == maxd).any() and (m == 1).any(), maxd
            if maxd == 32 * k + 2:                               # the single live candidate of its tile: lane column 0
                cols = (np.argwhere(m == maxd)[:, 1]) % 32
                assert (cols == 0).any(), maxd
