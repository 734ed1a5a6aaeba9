"""The algebra of the matrix-core SSD kernel (csrc/ws_march_mfma.h), step by step in numpy against a brute-force SSD
argmin -- a witness that needs no device:

  * signed bytes a^ = a xor 0x80, one row of the window = 3 * WW contiguous bytes, K padded to 32 with the pad zeroed on
    ONE operand (after the complement);
  * 32 x 32 tiles, rows = target centres v, columns = outputs x; int32 accumulators that wrap;
  * per step the entering row with the A side complemented, the leaving row plain:
    Acc = -(cross sum over the window) - E(v);
  * bias'[v] = ((window sum of b^^2) + 2 E(v)) << KT + tag from running per-centre sums, key = (Acc << (KT + 1)) + bias'
    modulo 2^32;
  * 4-bit tags inside groups of 16 candidates (register order = disparity order, the preferred disparity first), a
    strict '<' on the cost words between groups taken in the preferred order.

Both tie rules are run: the smaller d (as the reference's right view) and the larger d (the left view, the one the
kernel is selected for).  A flat region makes every candidate of a pixel tie, 0 / 255 inputs sit at the int8 limits.
"""
import numpy as np
import pytest

WW = WH = 7
KT = 4


def _pair(kind, h=30, w=120):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(np.roll(a, -5, 1).astype(int) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    if kind == "flat":                 # every candidate of a pixel in the region ties
        a[5:20, 60:90] = 7
        b[5:20, 40:90] = 7
    elif kind == "limits":             # 255 against 0: -128 / 127 and the complement at the int8 limits
        a[:, 50:] = 255
        b[:, :70] = 0
        b[8:12, 20:40] = 255
    return a, b


def _brute(a, b, D, prefer_large):
    """Top-left anchored windows: output (y, x) for x in [D - 1, W - WW], candidate d in [0, D) looks at v = x - d."""
    h, w = a.shape[:2]
    out = np.full((h - WH + 1, w), -1)
    ai, bi = a.astype(np.int64), b.astype(np.int64)
    order = range(D - 1, -1, -1) if prefer_large else range(D)
    for y in range(h - WH + 1):
        for x in range(D - 1, w - WW + 1):
            best = None
            for d in order:            # the first candidate of the preferred order keeps a tie (strict '<')
                v = x - d
                c = ((ai[y:y + WH, x:x + WW] - bi[y:y + WH, v:v + WW]) ** 2).sum()
                if best is None or c < best:
                    best, out[y, x] = c, d
    return out


def _operand(raw, row, c0, n, comp=False, mask=False):
    """n rows of an operand: 32 bytes each from byte 3 * (c0 + r) of the raw row (zeros past its end)."""
    o = np.zeros((n, 32), np.int8)
    for r in range(n):
        seg = raw[row, 3 * (c0 + r):3 * (c0 + r) + 32]
        o[r, :len(seg)] = seg
    if comp:
        o = ~o
    if mask:
        o[:, 3 * WW:] = 0              # the pad, after the complement: on this side it must be zero
    return o.astype(np.int32)


def _emulate(a, b, D, prefer_large):
    h, w = a.shape[:2]
    raw_a = (a ^ 0x80).view(np.int8).reshape(h, 3 * w)
    raw_b = (b ^ 0x80).view(np.int8).reshape(h, 3 * w)
    bh = (b ^ 0x80).view(np.int8).astype(np.int64)
    xs = np.arange(D - 1, w - WW + 1)
    vs = np.arange(xs[0] - (D - 1), xs[-1] + 1)
    x0, v0, nx, nv = xs[0], vs[0], len(xs), len(vs)
    acc = np.zeros((nv, nx), np.int32)                         # rows v (MFMA M), columns x (MFMA N = the lane)
    bsq, bsum = (bh ** 2).sum(2), bh.sum(2)
    win = lambda arr, row: np.array([arr[row, v:v + WW].sum() for v in vs])
    G = np.zeros(nv, np.int64)                                 # window sum of b^^2
    E = np.zeros(nv, np.int64)                                 # sum of b^ over every row entered so far
    out = np.full((h - WH + 1, w), -1)
    for row in range(h):
        a_e, b_e = _operand(raw_a, row, x0, nx, comp=True, mask=True), _operand(raw_b, row, v0, nv)
        with np.errstate(over="ignore"):
            acc = (acc + (b_e @ a_e.T).astype(np.int32)).astype(np.int32)
        G += win(bsq, row)
        E += win(bsum, row)
        if row >= WH:
            a_l, b_l = _operand(raw_a, row - WH, x0, nx, mask=True), _operand(raw_b, row - WH, v0, nv)
            with np.errstate(over="ignore"):
                acc = (acc + (b_l @ a_l.T).astype(np.int32)).astype(np.int32)
            G -= win(bsq, row - WH)
        if row < WH - 1:
            continue
        bias = (G + 2 * E) << KT
        groups = range(0, D, 16)
        for xi, x in enumerate(xs):
            best = None
            for g0 in (reversed(groups) if prefer_large else groups):
                kmin = None
                for d in range(g0, min(D, g0 + 16)):
                    vi = x - d - v0
                    tag = (min(D, g0 + 16) - 1 - d) if prefer_large else d - g0
                    key = ((int(acc[vi, xi]) << (KT + 1)) + int(bias[vi]) + tag) & 0xffffffff
                    key -= (1 << 32) if key >= (1 << 31) else 0
                    kmin = key if kmin is None or key < kmin else kmin
                if best is None or (kmin >> KT) < (best[0] >> KT):
                    best = (kmin, g0)
            kmin, g0 = best
            tag = kmin & 15
            out[row - (WH - 1), x] = (min(D, g0 + 16) - 1 - tag) if prefer_large else g0 + tag
    return out


@pytest.mark.parametrize("prefer_large", [False, True])
@pytest.mark.parametrize("kind", ["flat", "limits"])
def test_matrix_formulation_equals_brute_force(kind, prefer_large):
    a, b = _pair(kind)
    D = 48
    want = _brute(a, b, D, prefer_large)
    got = _emulate(a, b, D, prefer_large)
    m = want >= 0
    assert m.sum() == 24 * (120 - WW + 1 - (D - 1))
    assert np.array_equal(got[m], want[m]), "%d of %d pixels differ" % ((got[m] != want[m]).sum(), m.sum())
    if kind == "flat":                 # the ties are really there: the preferred end of the tying candidates wins -- d = 0,
        #                                or the largest d whose window still lies in the target's flat columns (from 40 on)
        assert (want[5:14, 60:84] == (np.arange(60, 84) - 40 if prefer_large else 0)).all()


def test_key_ranges():
    """A centred cost word sum b^^2 - 2 sum a^.b^ lies in [-128^2, 128^2 + 2 * 127 * 128] per byte of the window; shifted
    by KT it must stay inside (-2^28, 2^28), the flush's validity test."""
    for ww in (7, 9):
        n = 3 * ww * ww
        lo, hi = -128 * 128 * n, (128 * 128 + 2 * 127 * 128) * n
        assert -(1 << 28) < (lo << KT) and ((hi << KT) + 15) < (1 << 28), ww
        # b^ = -128 everywhere, a^ = 127: the top is reached; a^ = b^ = -128: sum b^2 - 2 sum ab = -128^2 n, the bottom
        assert (128 * 128 - 2 * 127 * -128) * n == hi and (128 * 128 - 2 * 128 * 128) * n == lo
