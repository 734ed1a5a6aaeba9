"""Pins tests/lr_ref.py -- the statement of the left-right check that the device is compared with -- on hand-built maps
whose results are worked out by hand from the rules in include/ws_stereo.h.  No device, no library."""
import numpy as np
import pytest

from lr_ref import EMPTY, FAILED, PASSED, lr_check, lr_states

F = np.float32
INF, NAN = np.inf, np.nan


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_consistent_maps_pass_and_an_occluded_strip_fails():
    # right map: every pixel x matches left column x + 2 (value 2); left map: value 2 except a strip [5, 8) of 4,
    # whose partners (x - 4) hold 2: |4 - 2| = 2 > 1.  Left x < 2 has its partner off the left edge.
    right = np.full((2, 12), 2, dtype=F)
    right[:, 10:] = 0                          # no disparity: x + 2 would leave the left map
    left = np.full((2, 12), 2, dtype=F)
    left[:, 5:8] = 4
    ol, orr, counts = lr_check(left, right, 1.0)
    want_l = left.copy()
    want_l[:, :2] = 0
    want_l[:, 5:8] = 0
    assert np.array_equal(ol, want_l)
    # right x passes iff left(x + 2) is within 1 of 2: x + 2 in [5, 8) holds 4
    want_r = right.copy()
    want_r[:, 3:6] = 0
    assert np.array_equal(orr, want_r)
    assert counts == (2 * 5, 2 * 3)
    # the strip is recovered with the farther surface when filled: both sides hold 2
    fl, _, fcounts = lr_check(left, right, 1.0, fill=True)
    want_fill = left.copy()
    want_fill[:, 5:8] = 2
    want_fill[:, :2] = 2                       # only the right side exists
    assert np.array_equal(fl, want_fill)
    assert fcounts == counts                   # filled pixels still count


def test_partners_off_either_edge_and_rows_beyond_the_partner():
    left = np.zeros((3, 6), dtype=F)
    right = np.zeros((2, 6), dtype=F)
    left[0, 1] = 2          # p = -1: off the left edge
    left[0, 4] = 3          # p = 1: partner 0 -> |3| > 1
    left[1, 3] = 1          # p = 2
    right[1, 2] = 1         # ... holds 1: pass
    right[0, 5] = 1         # p = 6 = w_L: off the right edge
    right[0, 0] = 5         # p = 5: last column, partner 0
    left[2, :] = [1, 2, 3, 1, 2, 3]   # row 2 >= h_R = 2: every non-empty pixel fails
    sl, sr = lr_states(left, right, 1.0)
    assert sl[0, 1] == FAILED and sl[0, 4] == FAILED and sl[1, 3] == PASSED
    assert (sl[2] == FAILED).all()
    assert sr[0, 5] == FAILED and sr[0, 0] == FAILED and sr[1, 2] == PASSED
    ol, orr, counts = lr_check(left, right, 1.0)
    assert counts == (2 + 6, 2)
    assert ol[1, 3] == 1 and orr[1, 2] == 1 and not ol[2].any()
    # an unequal width: a right map narrower than the left one
    ol, orr, counts = lr_check(np.array([[0, 0, 0, 0, 1]], F), np.array([[0, 0, 0, 1]], F), 0.0)
    assert counts == (0, 0) and ol[0, 4] == 1 and orr[0, 3] == 1


def test_rint_rounds_half_to_even():
    right = np.zeros((1, 8), dtype=F)
    right[0, 3] = 2.5       # 2.5 at x = 5 rounds to 2: partner 3
    right[0, 2] = 100       # ... not 2 (round half up would land here)
    right[0, 1] = 3.5       # 3.5 at x = 5 rounds to 4: partner 1
    left = np.zeros((1, 8), dtype=F)
    left[0, 5] = 2.5
    sl, _ = lr_states(left, right, 0.0)
    assert sl[0, 5] == PASSED
    left[0, 5] = 3.5
    sl, _ = lr_states(left, right, 0.0)
    assert sl[0, 5] == PASSED
    right[0, 3] = 0
    right[0, 1] = 0
    for v, p in ((2.5, 2), (3.5, 4), (-0.5, 0), (0.5, 0), (1.5, 2)):   # the right map: p = x + rint(v)
        r = np.zeros((1, 8), dtype=F)
        r[0, 1] = v
        lm = np.zeros((1, 8), dtype=F)
        lm[0, 1 + int(np.rint(v))] = v
        assert 1 + int(np.rint(v)) == 1 + p
        _, sr = lr_states(lm, r, 0.0)
        assert sr[0, 1] == PASSED, v


def test_signed_zero_nan_and_infinities():
    left = np.array([[-0.0, NAN, INF, -INF, 1, 1, 1]], dtype=F)
    right = np.array([[0.0, 0.0, 0.0, NAN, INF, 1.0, 0.0]], dtype=F)
    sl, sr = lr_states(left, right, 1.0)
    assert sl[0, 0] == EMPTY                   # -0.0 is "no disparity"
    assert (sl[0, 1:4] == FAILED).all()        # NaN, +inf, -inf fail
    assert sl[0, 4] == FAILED                  # partner (x = 3) is NaN
    assert sl[0, 5] == FAILED                  # partner (x = 4) is +inf: |1 - inf| > 1
    assert sl[0, 6] == PASSED                  # partner (x = 5) is 1
    assert sr[0, 3] == FAILED and sr[0, 4] == FAILED
    assert sr[0, 5] == PASSED                  # v = 1: partner left(6) = 1
    ol, orr, counts = lr_check(left, right, 1.0)
    assert bits(ol)[0, 0] == 0                 # the output is +0.0
    assert counts == (5, 2)
    assert ol[0, 6] == 1 and orr[0, 5] == 1
    # with max_diff = +inf an infinite difference passes, a NaN one does not
    sl, _ = lr_states(left, right, np.inf)
    assert sl[0, 5] == PASSED and sl[0, 4] == FAILED


def test_max_diff_zero_and_infinity():
    left = np.array([[0, 0, 3, 0, 0, 2]], dtype=F)
    right = np.array([[0, 0, 0, 3.5, 0, 0]], dtype=F)
    # left x = 5, v = 2: partner right(3) = 3.5, |2 - 3.5| = 1.5; left x = 2, v = 3: partner -1 (off the edge)
    for md, want in ((0.0, FAILED), (1.5, PASSED), (1.4999, FAILED), (np.inf, PASSED)):
        sl, _ = lr_states(left, right, md)
        assert sl[0, 5] == want, md
        assert sl[0, 2] == FAILED
    # a partner of 0 fails unless |v| <= max_diff
    left = np.array([[0, 0, 0, 2.0]], dtype=F)
    right = np.zeros((1, 4), dtype=F)
    assert lr_states(left, right, 1.0)[0][0, 3] == FAILED
    assert lr_states(left, right, 2.0)[0][0, 3] == PASSED
    assert lr_states(left, right, np.inf)[0][0, 3] == PASSED
    ol, _, counts = lr_check(left, right, 0.0)
    assert counts == (1, 0) and not ol.any()
    with pytest.raises(ValueError):
        lr_check(left, right, -1.0)
    with pytest.raises(ValueError):
        lr_check(left, right, np.nan)


def test_fill_with_one_side_both_sides_or_none():
    # left map row 0: passed at x = 2 (value 2, partner right(0) = 2) and x = 7 (value 1, partner right(6) = 1)
    left = np.zeros((2, 10), dtype=F)
    right = np.zeros((2, 10), dtype=F)
    left[0, 2], right[0, 0] = 2, 2
    left[0, 7], right[0, 6] = 1, 1
    left[0, 0] = 9          # fails (off the edge): only a right source (x = 2) -> 2
    left[0, 4] = 9          # fails: both sides (2 and 1) -> fminf = 1
    left[0, 5] = -0.0       # empty: stays 0, is not a source
    left[0, 9] = 9          # fails: only a left source (x = 7) -> 1
    left[1, 3] = 9          # row 1: fails, no source at all -> 0
    ol, orr, counts = lr_check(left, right, 0.0, fill=True)
    assert ol[0].tolist() == [2, 0, 2, 0, 1, 0, 0, 1, 0, 1]
    assert not ol[1].any()
    assert counts[0] == 4
    # filled pixels never feed others: a failed pixel between a filled one and nothing gets the passed value only
    ol0, _, _ = lr_check(left, right, 0.0, fill=False)
    assert ol0[0].tolist() == [0, 0, 2, 0, 0, 0, 0, 1, 0, 0]
    # the right map's failed pixels are filled the same way (right(0) = 2 -> p = 2 holds 2 -> passes)
    assert orr[0, 0] == 2 and orr[0, 6] == 1


def test_random_maps_agree_with_a_per_pixel_loop():
    """The row-at-once statement against the rules written out one pixel at a time."""
    rng = np.random.default_rng(3)
    for trial in range(20):
        hl, wl, hr, wr = rng.integers(1, 6), rng.integers(1, 20), rng.integers(1, 6), rng.integers(1, 20)
        left = rng.choice(np.array([0, -0.0, 1, 2, 2.5, 3.5, -1, NAN, INF, -INF, 4], dtype=F), size=(hl, wl))
        right = rng.choice(np.array([0, 1, 2, 2.5, 3.5, -2, NAN, INF, 4, 1.5], dtype=F), size=(hr, wr))
        md = float(rng.choice([0.0, 0.5, 1.0, np.inf]))
        for fill in (False, True):
            ol, orr, counts = lr_check(left, right, md, fill)
            wl_, wr_, c = _loop(left, right, md, fill)
            assert np.array_equal(bits(ol), bits(wl_)) and np.array_equal(bits(orr), bits(wr_)) and counts == c


def _loop(left, right, md, fill):
    outs, counts = [], []
    for a, b, s in ((left, right, -1), (right, left, 1)):
        h, w = a.shape
        out = np.zeros((h, w), dtype=F)
        st = np.zeros((h, w), dtype=np.uint8)
        for y in range(h):
            for x in range(w):
                v = a[y, x]
                if v == 0:
                    continue
                ok = False
                if np.isfinite(v) and y < b.shape[0]:
                    p = x + s * int(np.rint(v))
                    if 0 <= p < b.shape[1]:
                        with np.errstate(invalid="ignore", over="ignore"):
                            ok = bool(np.abs(F(v) - F(b[y, p])) <= F(md))
                st[y, x] = PASSED if ok else FAILED
                out[y, x] = v if ok else 0
        if fill:
            src = out.copy()
            for y in range(h):
                for x in range(w):
                    if st[y, x] != FAILED:
                        continue
                    lv = next((src[y, i] for i in range(x - 1, -1, -1) if st[y, i] == PASSED), None)
                    rv = next((src[y, i] for i in range(x + 1, w) if st[y, i] == PASSED), None)
                    out[y, x] = min(lv, rv) if lv is not None and rv is not None else lv if lv is not None else rv if rv is not None else 0
        outs.append(out)
        counts.append(int((st == FAILED).sum()))
    return outs[0], outs[1], tuple(counts)
