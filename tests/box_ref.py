"""Two independent statements of removeDisparityOutliers (reconstruction.cpp:5-18) that are exact for fractional maps,
and a bound on what the device's double path may add to them.  Test infrastructure only.

The operation, restated: for a float32 map A, a kernel size k >= 1 and two float32 thresholds,
  1. s(y, x) = the sum of the k x k window anchored at (k // 2, k // 2) of the BORDER_REFLECT_101 extension of A,
     as a real number;
  2. blurred = float32(double(s) * (1 / (double(k) * double(k))))  -- cv::blur's CV_32F path: double sums, one
     multiplication by the reciprocal, one cast;
  3. a pixel with A > thr_front * blurred or A < thr_back * blurred (float32 products, float32 comparisons) takes
     blurred, every other pixel keeps its bits.

outliers_exact   NumPy, int64: the map in units of 2^-S, separable cumulative sums over a reflected index vector.
outliers_literal plain Python, one pixel and one window element at a time, reflect101 as the `while` loop, the sum a
                 fractions.Fraction: exact for any finite float32 input; for tiny maps.
blur_interval    for maps the device cannot sum exactly: the float32 values the blur may take.

oracle.remove_disparity_outliers is not used for fractional maps: its float64 2-D cumulative sum rounds (at 3840 x 2160,
k = 31, multiples of 2^-23 below 300 it differs from the exact filter, test_box_reference.py pins the example).


What the device's double path forms (ws_consumers.hip: ws_box_rows_kernel, ws_outlier_cols_kernel, ext_prefix,
ext_window and the two direct kernels), per line of n elements with L = the sum of their magnitudes:

  * the scans: sums of runs of consecutive elements, magnitude <= L;
  * ext_prefix(t), q = t // (2n - 2), r = t % (2n - 2):
        r <= n, q = 0:  P[r]                                    every element counted at most once      <= L
        r > n:          P[n] + P[n-1] - P[2n-1-r]               at most twice                           <= 2 L
        q >= 1:         q * (P[n] + P[n-1] - P[1]) + g          at most 2 q + 2 times                   <= (2q + 2) L
    so |ext_prefix(t)| and every partial result inside it is <= c(t) L, c(t) = 1 if t <= n and t < 2n - 2 (a line of two
    elements has 2n - 2 = n), else 2 (t // (2n-2)) + 2, and c is non-decreasing in t;
  * ext_window, x0 >= 0: ext_prefix(x0 + k) - ext_prefix(x0) with x0 + k <= n - 1 - k // 2 + k =: tA; the difference
    counts no element more often than its first operand                                       <= c(tA) L
  * ext_window, x0 < 0 (k >= 2): (ext_prefix(-x0 + 1) - P[1]) + ext_prefix(x0 + k) with -x0 + 1 <= k // 2 + 1 and
    x0 + k <= k - 1                                                                           <= (c(k//2 + 1) + c(k - 1)) L
  * n = 1: k * P[1]                                                                           <= k L
  * the direct kernels add the window's k elements one by one; every element is met at most 2 ceil(k / (2n-2)) times,
    which is below the counts above.

Q(n, k) = max(c(tA), c(k//2 + 1) + c(k - 1)) (k for n = 1) therefore bounds every intermediate of a line by Q L.  The
column pass runs on the row sums, whose magnitudes are at most the k-wide window sums R of |A|; a column of them has
L_col = sum over y of R(y, x).  When every value of the map is an integer multiple of 2^-S, every intermediate is an
integer in those units, and a double addition, subtraction or multiplication by q of integers is exact when the result
is below 2^53.  Hence

    exact_on_device  <=>  Q(w, k) * max_y L_row(y) * 2^S < 2^53  and  Q(h, k) * max_x L_col(x) * 2^S < 2^53.

(The issue's rough form 2 (max(w, h) + k + 1) k max|v| 2^S < 2^53 bounds L_col by h k max|v| and Q by 2 (1 + k / n);
this one uses the map's own sums.)


The rounding bound E of blur_interval, for maps outside that domain.  u = 2^-53; every double operation adds at most
u times the magnitude of its result, which the above bounds by M = Q L (1 + 2^-40) -- the factor covers the computed
magnitudes differing from the exact ones by the very errors being bounded.
  * a prefix value P[r] of the row kernel: the thread's own run (per - 1 additions, per = ceil(w / 256)), the wave scan
    (6), the wave totals (3), `incl - v` and `before +` (2), the thread's run again (per): A_row = 2 per + 10 additions;
  * of the column kernel: 31 + 6 + 15 + 1 + 32: A_col = 85 additions;
  * ext_prefix reads at most 3 values for g and 3 for the period, the latter multiplied by q, and makes 2 + 2 q + 2
    operations (the period's two count q times); ext_window takes two of them, P[1] and two more operations: at most
    NP = 6 q + 7 weighted prefix values and NO = 4 q + 10 operations, q = tA // (2n - 2);
  * the direct kernels make k additions.
    N(line) = max(NP * A + NO, k),  E_row = N(row) u M_row
  * the column pass sums row sums that are each off by at most E_row; its result is a sum of exactly k of them, so they
    contribute k E_row;                        E = k E_row + N(col) u M_col.
The device then forms float32(double(acc * scale)): one more double rounding.  Acceptable float32 results are
float32((s - E) scale (1 -+ u)) .. float32((s + E) scale (1 +- u)) and whatever lies between; blur_interval evaluates
the ends in float64 from the exact integer s and pushes each outwards by four float64 ulps, which only widens it.
"""
from fractions import Fraction

import numpy as np

_TWO53 = 1 << 53


def _map(a):
    a = np.array(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("expected a non-empty H x W map")
    if not np.isfinite(a).all():
        raise ValueError("the exact references take finite maps only")
    return a


def scale_bits(a):
    """The smallest S >= 0 such that every value of the float32 map is an integer multiple of 2^-S."""
    f, e = np.frexp(a.astype(np.float64))                 # a = f * 2^e, 0.5 <= |f| < 1, 24 significant bits
    m = np.abs(np.ldexp(f, 24)).astype(np.int64)          # the 24-bit significand as an integer: a = +-m * 2^(e - 24)
    nz = m != 0
    if not nz.any():
        return 0
    m, e = m[nz], e[nz].astype(np.int64)
    tz = np.zeros_like(m)
    low = m & -m                                          # the lowest set bit
    for b in (16, 8, 4, 2, 1):
        big = low >= (1 << b)
        tz[big] += b
        low[big] >>= b
    return int(max(0, (24 - e - tz).max()))


def _reflect_index(n, k):
    """Indices into a line of n elements of its REFLECT_101 extension at -k//2 .. n + k - 2 - k//2."""
    i = np.arange(-(k // 2), n + k - 1 - (k // 2), dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    t = 2 * n - 2
    i = np.mod(i, t)
    return np.where(i >= n, t - i, i)


def _window_sums(ints, k, axis):
    """The k-long window sums of the extended lines of an int64 array along `axis`."""
    n = ints.shape[axis]
    ext = np.take(ints, _reflect_index(n, k), axis=axis)
    c = np.cumsum(ext, axis=axis, dtype=np.int64)
    pad = [(0, 0), (0, 0)]
    pad[axis] = (1, 0)
    c = np.pad(c, pad)
    hi = [slice(None), slice(None)]
    lo = [slice(None), slice(None)]
    hi[axis], lo[axis] = slice(k, k + n), slice(0, n)
    return c[tuple(hi)] - c[tuple(lo)]


def _ints(a, k):
    s_bits = scale_bits(a)
    top = int(np.abs(a.astype(np.float64)).max() * 2.0 ** s_bits) + 1
    if top * k * k >= 1 << 62:
        raise ValueError("2^-%d units x %d x %d windows do not fit int64" % (s_bits, k, k))
    return np.ldexp(a.astype(np.float64), s_bits).astype(np.int64), s_bits


def _c(t, n):
    return 1 if t <= n and t < 2 * n - 2 else 2 * (t // (2 * n - 2)) + 2


def line_factor(n, k):
    """Q(n, k) of the module docstring: no intermediate of a line counts an element more often than this."""
    if n == 1:
        return k
    q = _c(n - 1 - k // 2 + k, n)
    if k >= 2:
        q = max(q, _c(k // 2 + 1, n) + _c(k - 1, n))
    return q


def device_magnitudes(a, k):
    """(Q_row * max L_row, Q_col * max L_col) in units of 2^-S, as Python ints, and S."""
    a = _map(a)
    ints, s_bits = _ints(a, k)
    mag = np.abs(ints)
    h, w = a.shape
    l_row = int(mag.sum(axis=1).max())
    l_col = int(_window_sums(mag, k, 1).sum(axis=0).max())
    return line_factor(w, k) * l_row, line_factor(h, k) * l_col, s_bits


def _rule(a, blurred, thr_front, thr_back):
    out = a.copy()
    bad = (a > np.float32(thr_front) * blurred) | (a < np.float32(thr_back) * blurred)
    out[bad] = blurred[bad]
    return out


def exact_window_sums(a, k):
    """(int64 k x k window sums in units of 2^-S, S)."""
    a = _map(a)
    k = int(k)
    if k < 1:
        raise ValueError("kernel size below 1")
    ints, s_bits = _ints(a, k)
    return _window_sums(_window_sums(ints, k, 1), k, 0), s_bits


def outliers_exact(disparity, kernel_size, thr_front, thr_back):
    """Returns (filtered float32 map, exact_on_device)."""
    a = _map(disparity)
    k = int(kernel_size)
    s, s_bits = exact_window_sums(a, k)
    blurred = (np.ldexp(s.astype(np.float64), -s_bits) * (1.0 / (float(k) * float(k)))).astype(np.float32)
    m_row, m_col, _ = device_magnitudes(a, k)
    return _rule(a, blurred, thr_front, thr_back), bool(m_row < _TWO53 and m_col < _TWO53)


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def outliers_literal(disparity, kernel_size, thr_front, thr_back):
    """The filtered float32 map, by the definition, one window element at a time."""
    a = _map(disparity)
    k = int(kernel_size)
    h, w = a.shape
    scale = 1.0 / (float(k) * float(k))
    tf, tb = np.float32(thr_front), np.float32(thr_back)
    out = a.copy()
    vals = [[Fraction(float(a[y, x])) for x in range(w)] for y in range(h)]
    for y in range(h):
        for x in range(w):
            s = Fraction(0)
            for j in range(k):
                row = vals[reflect101(y - k // 2 + j, h)]
                for i in range(k):
                    s += row[reflect101(x - k // 2 + i, w)]
            blurred = np.float32(float(s) * scale)          # Fraction.__float__ rounds correctly, ties to even
            d = a[y, x]
            if d > tf * blurred or d < tb * blurred:
                out[y, x] = blurred
    return out


def _ops(n, k, adds):
    if n == 1:
        return max(1, k)
    q = (n - 1 - k // 2 + k) // (2 * n - 2)
    return max((6 * q + 7) * adds + 4 * q + 10, k)


def rounding_bound(a, k):
    """E of the module docstring in units of 2^-S (a float, rounded up), and S."""
    a = _map(a)
    h, w = a.shape
    m_row, m_col, s_bits = device_magnitudes(a, k)
    u, slack = 2.0 ** -53, 1.0 + 2.0 ** -40
    per = -(-w // 256)
    e_row = _ops(w, k, 2 * per + 10) * u * float(m_row) * slack
    e = k * e_row + _ops(h, k, 85) * u * float(m_col) * slack
    return e * (1.0 + 2.0 ** -50), s_bits


def _outwards(x, down):
    for _ in range(4):
        x = np.nextafter(x, -np.inf if down else np.inf)
    return x


def blur_interval(disparity, kernel_size):
    """(lo, hi, blurred): float32 maps; the device's blur must lie in [lo, hi]; blurred is the exact filter's."""
    a = _map(disparity)
    k = int(kernel_size)
    s, s_bits = exact_window_sums(a, k)
    if int(np.abs(s).max()) >= 1 << 62:
        raise ValueError("window sums too large")
    e, _ = rounding_bound(a, k)
    scale = 1.0 / (float(k) * float(k))
    sf = s.astype(np.float64)
    e = e + np.where(np.abs(s) >= _TWO53, np.abs(sf) * 2.0 ** -52, 0.0)   # int64 -> float64 rounds there: widen by it
    u = 2.0 ** -53
    ends = []
    for sign in (-1.0, 1.0):
        v = np.ldexp(sf + sign * e, -s_bits) * scale
        ends.append(_outwards(np.minimum(v * (1.0 - u), v * (1.0 + u)), True))
        ends.append(_outwards(np.maximum(v * (1.0 - u), v * (1.0 + u)), False))
    lo = np.minimum.reduce(ends).astype(np.float32)
    hi = np.maximum.reduce(ends).astype(np.float32)
    blurred = (np.ldexp(sf, -s_bits) * scale).astype(np.float32)
    return lo, hi, blurred
