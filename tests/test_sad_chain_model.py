"""A NumPy model of the SSD marching kernel's v_sad_u32 chain (ws_march_kernel.h, march_sadp / march_sadp_halo and the
bias stage in produce), computed modulo 2^32 the way the device computes it: the entering row's reference pixels
complemented, the leaving row's plain, one |hi - lo| + P per window update, the key (P << (KT + 1)) + bias' + tag,
the merge slot's (cost word, tag word) and the flush's decoding.  Every key must equal (sum b^2 - 2 sum a.b) << KT +
tag exactly, and the winner, its disparity and its cost must be those of the shifted chain it replaces (keys
(cost << log2 ND) + local tag, slot tag word local tag | chunk tag) -- on random rows, all-0 and all-255 rows, and
inputs where every candidate ties, for both tie rules, at 7 x 7 and 9 x 9, with several d-chunks and poisoned
candidates.
"""
import numpy as np
import pytest

M32 = (1 << 32) - 1
K_POISON = 1 << 29
K_VALID = 1 << 28
X = 8


def _tag_bits(x, nd):                       # ws_device.h: ssd_sad_tag_bits
    return int(2 * (x + nd - 1) - 1).bit_length() - 1


def _i32(v):
    v = np.asarray(v, dtype=np.int64) & M32
    return np.where(v >= 1 << 31, v - (1 << 32), v)


def _dot(a, b):
    """v_dot4_u32_u8 of pixel arrays (..., 3): the 4th byte of b is 0"""
    return (a.astype(np.int64) * b.astype(np.int64)).sum(axis=-1)


def _images(kind, rng, rows, na, nb):
    if kind == "random":
        return rng.integers(0, 256, (rows, na, 3)), rng.integers(0, 256, (rows, nb, 3))
    if kind == "zeros":
        return np.zeros((rows, na, 3), np.int64), np.zeros((rows, nb, 3), np.int64)
    if kind == "full":
        return np.full((rows, na, 3), 255), np.full((rows, nb, 3), 255)
    if kind == "extremes":                   # 0 against 255: the largest costs
        return np.zeros((rows, na, 3), np.int64), np.full((rows, nb, 3), 255)
    if kind == "constant":                   # every candidate of a pixel ties
        v = int(rng.integers(0, 256))
        return np.full((rows, na, 3), v), np.full((rows, nb, 3), v)
    if kind == "periodic":                   # ties between candidates one period apart
        a = np.tile(rng.integers(0, 256, (rows, 1, 3)), (1, na, 1))
        b = np.tile(rng.integers(0, 256, (rows, 1, 3)), (1, nb, 1))
        return a, b
    raise ValueError(kind)


def _run(ww, wh, nd, nch, kind, prefer_large, halo, seed):
    rng = np.random.default_rng(seed)
    lt, kt = int(nd).bit_length() - 1, _tag_bits(X, nd)
    na, dt = X + ww - 1, nch * nd
    nbg = na + dt - 1                       # the target columns all chunks read
    steps = wh + 4                          # warm-up, the first output row, steady rows
    A, B = _images(kind, rng, steps, na, nbg)
    d_hi = dt - 1 - int(rng.integers(0, nd))  # a partly filled last chunk: candidates beyond d_hi are poisoned
    bad_k = set(rng.choice(nbg, size=2, replace=False).tolist())  # target centres outside [b_lo, b_hi]
    tmask = (1 << kt) - 1 if prefer_large else 0
    nbias = X + nd - 1
    # the shifted chain's winner per (row, x) and the new one, both as (cost word, tag word) 64-bit slots
    old_best, new_best = {}, {}
    for c in range(nch):
        d0 = c * nd
        # pb[m] of this chunk = global target column m + dt - nd - d0
        off = dt - nd - d0
        pb_cols = np.arange(na + nd - 1) + off
        P = np.zeros((X, nd), np.int64)
        for j in range(nd):
            if d0 + j > d_hi:
                P[:, j] = K_POISON >> (kt + 1)
        G = np.zeros(na + nd - 1, np.int64)  # column sums over this chunk's target columns, without the constant
        ctag = (dt - 1) - d0 - (nd - 1) if prefer_large else d0
        for a in range(steps):
            ca = 255 - A[a]                  # the twin of ring A: the entering row complemented
            pbr = B[a][pb_cols]
            if a >= wh:
                la, qbr = A[a - wh], B[a - wh][pb_cols]
            # the bias stage: the entering row's (255 - b)^2, the leaving row's b^2
            G = G + ((255 - pbr) ** 2).sum(axis=-1)
            if a >= wh:
                G = G - (qbr ** 2).sum(axis=-1)
            for j in range(nd):
                idx = np.arange(na) - j + nd - 1
                terms = _dot(ca, pbr[idx])
                if a >= wh:
                    terms = terms + _dot(la, qbr[idx])
                assert (terms >= 0).all()
                S = np.cumsum(terms) & M32
                assert S[-1] < 1 << 23
                for x in range(X):
                    lo = S[x - 1] if x else 0
                    if halo and x + ww - 1 >= X:  # T = S[X-1] + the next run's prefix (its own columns from X on)
                        hi = (S[X - 1] + (S[x + ww - 1] - S[X - 1])) & M32
                    else:
                        hi = S[x + ww - 1]
                    P[x, j] = (abs(int(hi) - int(lo)) + int(P[x, j])) & M32  # v_sad_u32
            if a < wh - 1:
                continue
            pre = np.concatenate([[0], np.cumsum(G)])
            cst = ((-(ww * 3 * 255 * 255) * (a + 1)) << kt) & M32
            bias = np.array([(((int(pre[k + ww] - pre[k]) << kt) + cst + (K_POISON if (k + off) in bad_k else 0)) & M32)
                             for k in range(nbias)], np.int64)
            rows = range(a - wh + 1, a + 1)
            for x in range(X):
                for j in range(nd):
                    k = x - j + nd - 1
                    tag = (X + nd - 2 - k) ^ tmask
                    key = int(_i32((int(P[x, j]) << (kt + 1)) + int(bias[k]) + tag))
                    # the exact key: sum b^2 - 2 sum a.b over the window, << KT, + tag, + poison
                    cols_a = np.arange(x, x + ww)
                    cols_b = cols_a - j + nd - 1 + off
                    cost = sum(int(((B[r][cols_b] ** 2).sum()) - 2 * int(_dot(A[r][cols_a], B[r][cols_b]).sum())) for r in rows)
                    poison = (K_POISON if d0 + j > d_hi else 0) + (K_POISON if (k + off) in bad_k else 0)
                    assert key == (cost << kt) + tag + poison, (x, j, key, cost)
                    assert abs(cost << kt) + tag < K_VALID
                    # the slot of the new chain and of the shifted chain
                    hi_n = key & ~((1 << kt) - 1)
                    lo_n = (key & ((1 << kt) - 1)) | (ctag << (kt - lt))
                    ltag = nd - 1 - j if prefer_large else j
                    key_o = (cost << lt) + ltag + poison
                    hi_o, lo_o = key_o | (nd - 1), (key_o & (nd - 1)) | ctag
                    for best, s in ((new_best, (hi_n, lo_n)), (old_best, (hi_o, lo_o))):
                        cur = best.get((a, x))
                        if cur is None or s < cur:
                            best[(a, x)] = s
    # the flush: the same disparity and the same cost, or "no valid candidate" for both
    for (a, x), (hi_n, lo_n) in new_best.items():
        hi_o, lo_o = old_best[(a, x)]
        assert (hi_n >= K_VALID) == (hi_o >= K_VALID)
        if hi_o >= K_VALID:
            continue
        gtag = ((lo_n >> kt) << lt) + (lo_n & ((1 << kt) - 1)) - (x + (1 << kt) - (X + nd - 1) if prefer_large else X - 1 - x)
        assert gtag == lo_o, (a, x, gtag, lo_o)
        assert hi_n >> kt == hi_o >> lt


@pytest.mark.parametrize("ww", [7, 9])
@pytest.mark.parametrize("kind", ["random", "zeros", "full", "extremes", "constant", "periodic"])
@pytest.mark.parametrize("prefer_large", [False, True])
def test_sad_chain_keys(ww, kind, prefer_large):
    _run(ww, ww, 8, 2, kind, prefer_large, halo=False, seed=ww * 100 + len(kind))


@pytest.mark.parametrize("kind", ["random", "constant", "extremes"])
@pytest.mark.parametrize("prefer_large", [False, True])
def test_sad_chain_keys_narrow_and_halo(kind, prefer_large):
    _run(7, 7, 4, 3, kind, prefer_large, halo=False, seed=7)   # 4 disparities per thread: 11 tags, still 4 bits
    _run(9, 9, 8, 2, kind, prefer_large, halo=True, seed=9)    # the halo-exchange form at 9 x 9


def test_sad_chain_shapes():
    """ws_device.h's rule: the chain runs at 7 x 7 and 9 x 9 (and below) with 4 tag bits, not where bytes are centred"""
    def needs_centring(ww, wh, nd):
        return 2 * ww * wh * 3 * 255 * 255 * nd >= 1 << 28

    def sad_chain(ww, wh, nd):
        return not needs_centring(ww, wh, nd) and ((255 * 255 * ww * wh * 3 + 1) << _tag_bits(X, nd)) <= K_VALID
    assert _tag_bits(8, 8) == 4 and _tag_bits(8, 4) == 4
    for nd in (8, 4):
        assert [w for w in range(2, 18) if sad_chain(w, w, nd)] == list(range(2, 10))
