"""tests/box_ref.py against itself and against oracle.remove_disparity_outliers where that one is exact (CPU only)."""
import numpy as np
import pytest

import box_ref
from oracle import oracle


def _tiny_maps():
    rng = np.random.default_rng(2024)
    out = []
    for (h, w) in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 5), (5, 1), (2, 7), (7, 2), (3, 3), (4, 6), (6, 5)):
        for kind in ("integers", "negative", "fractions", "thirds"):
            if kind == "integers":
                m = rng.integers(0, 256, size=(h, w)).astype(np.float32)
            elif kind == "negative":
                m = rng.integers(-40, 300, size=(h, w)).astype(np.float32)
            elif kind == "fractions":
                m = (rng.integers(-(1 << 20), 1 << 20, size=(h, w)) / 4096.0).astype(np.float32)
            else:
                m = (rng.integers(1, 900, size=(h, w)) / 3.0).astype(np.float32)
            out.append((kind, m))
    return out


def test_exact_equals_literal_on_tiny_maps():
    n = 0
    for i, (kind, m) in enumerate(_tiny_maps()):
        h, w = m.shape
        # k from 1 to several periods 2n - 2 of either axis, even and odd
        for k in sorted({1, 2, 3, 4, 2 * max(w, h) - 2 + (i % 2), 4 * max(w, h) + 1 + (i % 2), 17 + i % 2}):
            if k < 1:
                continue
            for (tf, tb) in ((1.5, 0.8), (-1.0, 0.8)):
                got, _ = box_ref.outliers_exact(m, k, tf, tb)
                want = box_ref.outliers_literal(m, k, tf, tb)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, m.shape, k, tf)
                n += 1
    assert n >= 36 * 4


def test_exact_equals_the_oracle_on_integer_maps():
    rng = np.random.default_rng(7)
    for (w, h, k, hi) in ((300, 220, 500, 256), (300, 220, 31, 256), (1, 40, 7, 256), (40, 1, 7, 256), (2, 2, 500, 256),
                          (257, 130, 129, 4096), (33, 2300, 11, 256), (4100, 3, 9, 256), (640, 480, 4, 70000)):
        m = rng.integers(0, hi, size=(h, w)).astype(np.float32)
        m[rng.random((h, w)) < 0.05] = 0
        got, exact = box_ref.outliers_exact(m, k, 1.5, 0.8)
        assert exact, (w, h, k)
        assert np.array_equal(got, oracle.remove_disparity_outliers(m, k, 1.5, 0.8)), (w, h, k)
        assert (got != m).any() or w * h < 100


def test_scale_bits():
    assert box_ref.scale_bits(np.array([[0.0, 3.0, -256.0]], np.float32)) == 0
    assert box_ref.scale_bits(np.array([[0.5, 3.0]], np.float32)) == 1
    assert box_ref.scale_bits(np.array([[17.25, 2.0 ** -12]], np.float32)) == 12
    assert box_ref.scale_bits(np.array([[np.float32(1.0) + np.float32(2.0 ** -23)]], np.float32)) == 23
    assert box_ref.scale_bits(np.array([[np.float32(1.0 / 3.0)]], np.float32)) == 25
    with pytest.raises(ValueError):
        box_ref.outliers_exact(np.array([[1.0, np.nan]], np.float32), 3, 1.5, 0.8)
    with pytest.raises(ValueError):                                           # a denormal: 2^-149 units pass int64
        box_ref.outliers_exact(np.array([[1.0, 1e-45]], np.float32), 3, 1.5, 0.8)


def test_the_float64_cumulative_oracle_is_not_exact_on_subpixel_maps():
    """3840 x 2160, k = 31, multiples of 2^-23 below 300: the float64 2-D cumulative sum of
    oracle.remove_disparity_outliers rounds, the int64 filter does not.  The pinned reason box_ref exists."""
    rng = np.random.default_rng(0)
    m = (rng.integers(0, 300 << 23, size=(2160, 3840)).astype(np.float64) / float(1 << 23)).astype(np.float32)
    assert box_ref.scale_bits(m) == 23
    got, exact = box_ref.outliers_exact(m, 31, -1.0, 0.8)                      # every pixel replaced: the blur itself
    old = oracle.remove_disparity_outliers(m, 31, -1.0, 0.8)
    differ = int((got != old).sum())
    print("pixels where the float64 cumulative oracle differs from the exact filter:", differ)
    assert exact                                                               # ... and the device would be exact here
    assert 1 <= differ <= 100
    # the exact filter is the one that is right: spot-check the differing pixels by the definition, in Python ints
    ys, xs = np.nonzero(got != old)
    ints = np.ldexp(m.astype(np.float64), 23).astype(np.int64)
    for y, x in list(zip(ys, xs))[:5]:
        s = 0
        for j in range(31):
            yy = box_ref.reflect101(int(y) - 15 + j, 2160)
            for i in range(31):
                s += int(ints[yy, box_ref.reflect101(int(x) - 15 + i, 3840)])
        assert got[y, x] == np.float32(float(s) / float(1 << 23) * (1.0 / (31.0 * 31.0)))


def test_exact_on_device_either_side_of_the_bound():
    # one row, k = 1: Q = 1, so the bound is the row's own sum of magnitudes, in units of 2^-S, against 2^53
    odd = np.float32(1.0) + np.float32(2.0 ** -23)                             # forces S = 23
    below = np.array([[odd, 2.0 ** 29, 2.0 ** 28]], np.float32)                # 2^52 + 2^51 + 2^23 + 1 units
    assert box_ref.scale_bits(below) == 23
    assert box_ref.outliers_exact(below, 1, 1.5, 0.8)[1] is True
    above = np.array([[odd, 2.0 ** 29, 2.0 ** 29]], np.float32)                # 2^53 + 2^23 + 1 units
    assert box_ref.outliers_exact(above, 1, 1.5, 0.8)[1] is False
    coarse = np.array([[1.0, 2.0 ** 29, 2.0 ** 29]], np.float32)               # the same magnitudes in units of 1
    assert box_ref.outliers_exact(coarse, 1, 1.5, 0.8)[1] is True
    # ... and k = 3 counts the neighbours of the border twice (Q = 2)
    assert box_ref.outliers_exact(below, 3, 1.5, 0.8)[1] is False
    # sub-pixel-like values, multiples of 2^-23 below 256: exact at k = 500 up to 3840 x 2160 (the map's own sums keep
    # it at 0.39 of 2^53, where 2 (max(w, h) + k + 1) k max|v| 2^S would refuse it), not at k = 3000
    rng = np.random.default_rng(1)
    for (w, h, k, want) in ((1500, 1000, 500, True), (3840, 2160, 500, True), (3840, 2160, 3000, False)):
        m = (rng.integers(128 << 23, 256 << 23, size=(h, w)).astype(np.float64) / float(1 << 23)).astype(np.float32)
        assert box_ref.scale_bits(m) >= 16
        m[0, 0] = np.float32(1.0) + np.float32(2.0 ** -23)
        mr, mc, s = box_ref.device_magnitudes(m, k)
        assert s == 23
        assert (mr < 2 ** 53 and mc < 2 ** 53) is want, (w, h, k, mr / 2 ** 53, mc / 2 ** 53)
    # the periodic form counts elements several times: the same map passes with a short window, fails with a long one
    m = np.full((4, 4), np.float32(2.0 ** 47), np.float32)
    assert box_ref.device_magnitudes(m, 3)[1] < 2 ** 53 <= box_ref.device_magnitudes(m, 40)[1]


def test_line_factor_counts_what_ext_prefix_forms():
    """Q(n, k) against a brute count: run ext_window's formulas on vectors of per-element counts."""
    def counts_prefix(n, t):
        T = 2 * n - 2
        q, r = divmod(t, T)
        P = lambda j: np.concatenate([np.ones(j, np.int64), np.zeros(n - j, np.int64)])
        worst = 0
        if r <= n:
            g = P(r)
        else:
            worst = int((P(n) + P(n - 1)).max())
            g = P(n) + P(n - 1) - P(2 * n - 1 - r)
        if q == 0:
            return g, max(worst, int(g.max(initial=0)))
        per = P(n) + P(n - 1) - P(1)
        worst = max(worst, int((P(n) + P(n - 1)).max()), int((q * per).max()))
        return q * per + g, max(worst, int((q * per + g).max()))

    for n in range(2, 9):
        for k in range(1, 40):
            worst = 0
            for x in range(n):
                x0 = x - k // 2
                if x0 >= 0:
                    a, wa = counts_prefix(n, x0 + k)
                    b, wb = counts_prefix(n, x0)
                    res = a - b
                    worst = max(worst, wa, wb)
                else:
                    a, wa = counts_prefix(n, -x0 + 1)
                    b, wb = counts_prefix(n, x0 + k)
                    P1 = np.concatenate([np.ones(1, np.int64), np.zeros(n - 1, np.int64)])
                    res = (a - P1) + b
                    worst = max(worst, wa, wb)
                assert res.min() >= 0 and res.sum() == k                        # it is the window: k elements
                want = np.zeros(n, np.int64)
                for i in range(k):
                    want[box_ref.reflect101(x0 + i, n)] += 1
                assert np.array_equal(res, want), (n, k, x)
                worst = max(worst, int(res.max()))
            assert worst <= box_ref.line_factor(n, k), (n, k, worst)


def test_blur_interval_holds_the_exact_blur_and_is_tight():
    rng = np.random.default_rng(3)
    m = (rng.integers(1, 900, size=(120, 160)) / 3.0).astype(np.float32)
    for k in (5, 31, 500):
        lo, hi, blurred = box_ref.blur_interval(m, k)
        assert (lo <= blurred).all() and (blurred <= hi).all()
        steps = hi.view(np.int32).astype(np.int64) - lo.view(np.int32)         # positive floats: ulps between the ends
        assert steps.max() <= 1 and (steps == 0).mean() > 0.99, (k, steps.max(), (steps == 0).mean())
        e, s = box_ref.rounding_bound(m, k)
        win, _ = box_ref.exact_window_sums(m, k)
        assert e / float(np.abs(win).min()) < 1e-9                             # derived, and around 1e-12 relative
