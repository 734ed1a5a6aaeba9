"""Two independent restatements of the census-transform matching cost of include/ws_stereo.h, for the tests.

TEST INFRASTRUCTURE ONLY.
  * transform_np / volume: NumPy.  The descriptors by shifted compares; the window costs built like
    oracle/brute.py:cost_volume_left and tests/test_subpixel_reference.py:cost_volume_right, with the popcount plane in
    place of the SSD / SAD pixel cost.  volume() returns what sgm_ref.volume returns, so sgm_ref.sgm_from_volume gives the
    block-search map (P1 = P2 = 0) and the SGM maps.
  * transform_py / search_py: literal loops in plain Python integers for tiny images: one pixel, one neighbour, one bit
    at a time; its own windows, candidates, ties and parabola.
"""
import numpy as np

from oracle import brute
from sgm_ref import sgm_from_volume

RADII = {"census5x5": (2, 2), "census9x7": (4, 3)}   # (rx, ry)
BITS = {"census5x5": 24, "census9x7": 62}


def grey(img):
    """Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 of an H x W x 3 uint8 BGR image, int64."""
    a = img.astype(np.int64)
    return (1868 * a[..., 0] + 9617 * a[..., 1] + 4899 * a[..., 2] + 8192) >> 14


def transform_np(img, cost):
    """The descriptors of a whole image as uint64 (H x W)."""
    rx, ry = RADII[cost]
    y = grey(img)
    h, w = y.shape
    out = np.zeros((h, w), dtype=np.uint64)
    k = 0
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            # centres (cy, cx) whose neighbour (cy + dy, cx + dx) lies inside the image
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y1 > y0 and x1 > x0:   # (a neighbourhood larger than the image: no such centre)
                less = y[y0 + dy:y1 + dy, x0 + dx:x1 + dx] < y[y0:y1, x0:x1]
                out[y0:y1, x0:x1] |= less.astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def popcount(a):
    """Bits set in each element of a uint64 array, int64."""
    b = np.ascontiguousarray(a, dtype=np.uint64).view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(axis=-1).astype(np.int64)


def _black(img):
    return (img == 0).all(axis=2)


def volume(L, R, view, block_size, min_disparity, max_disparity, cost):
    """(vol [nd, h, w] int64 with -1 where d is no candidate, d0, node mask, region mask, black mask) of the view's map,
    as sgm_ref.volume.  Disparities no pixel can have (beyond the image's width) are left out: they are no candidates."""
    TL, TR = transform_np(L, cost), transform_np(R, cost)
    h1, w1 = L.shape[:2]
    h2, w2 = R.shape[:2]
    rows = min(h1, h2)
    half = (block_size - 1) // 2
    if view == "left":
        nd = max(0, min(max_disparity, w1 - 1))
        vol = np.full((nd, h1, w1), -1, dtype=np.int64)
        ys = np.arange(half, rows - half)
        for d in range(1, nd + 1):
            x_lo, x_hi = d, min(w1, w2 + d)
            if x_hi <= x_lo:
                continue
            s = brute._sat(popcount(TL[:rows, x_lo:x_hi] ^ TR[:rows, x_lo - d:x_hi - d]))
            xs = np.arange(half, w1 - half)
            cx = xs - d
            xs = xs[(cx >= half) & (cx < w2 - half)]
            if xs.size == 0 or ys.size == 0:
                continue
            a = xs - half - x_lo
            b = a + block_size
            top = (ys - half)[:, None]
            bot = top + block_size
            vol[d - 1][np.ix_(ys, xs)] = s[bot, b[None, :]] - s[top, b[None, :]] - s[bot, a[None, :]] + s[top, a[None, :]]
        d0, h, w = 1, h1, w1
        region = np.zeros((h1, w1), bool)
        region[half:rows - half, half:w1 - half] = True
        blk = _black(L)
    else:
        assert min_disparity >= 0 or max_disparity <= min_disparity
        hi = min(max_disparity, w1)
        nd = max(0, hi - min_disparity) if max_disparity > min_disparity else 0
        vol = np.full((nd, h2, w2), -1, dtype=np.int64)
        ys, xs = np.mgrid[0:rows, 0:w2]
        left, right = np.minimum(xs, half), np.minimum(w2 - xs - 1, half)
        up, down = np.minimum(ys, half), np.minimum(h2 - ys - 1, half)
        area = (left + right) * (up + down)
        for d in range(min_disparity, min_disparity + nd):
            n = min(w2, w1 - d)
            if n <= 0:
                break
            plane = np.zeros((rows, w2), dtype=np.int64)
            plane[:, :n] = popcount(TL[:rows, d:d + n] ^ TR[:rows, :n])
            s = brute._sat(plane)
            valid = (xs + d + right < w1) & (area > 0)
            y0, y1 = ys - up, np.minimum(ys + down, rows)
            x0, x1 = xs - left, xs + right
            win = s[y1, x1] - s[y0, x1] - s[y1, x0] + s[y0, x0]
            vol[d - min_disparity, :rows][valid] = win[valid]
        d0, h, w = min_disparity, h2, w2
        region = np.zeros((h2, w2), bool)
        region[:rows] = True
        blk = _black(R)
    valid = vol >= 0
    node = region & ~blk & valid.any(axis=0) if vol.shape[0] else np.zeros((h, w), bool)
    return vol, d0, node, region, blk


def slice_volume(V, nd):
    """What volume() returns for a smaller max_disparity (the first nd disparities), from the volume of a larger one: a
    pixel's candidates and their costs do not depend on max_disparity beyond the cut itself."""
    vol, d0, node, region, blk = V
    vol = vol[:max(0, nd)]
    node = region & ~blk & (vol >= 0).any(axis=0) if vol.shape[0] else np.zeros(node.shape, bool)
    return vol, d0, node, region, blk


def wta(V, view, subpixel=False):
    """sgm_from_volume(V, view, paths, 0, 0, subpixel) without walking the paths (with P1 = P2 = 0, S = paths * C: the
    same winner, and the parabola's quotient is unchanged by the power-of-two factor)."""
    vol, d0, node, region, blk = V
    nd = vol.shape[0]
    h, w = node.shape
    xs = np.broadcast_to(np.arange(w)[None, :], (h, w))
    out = np.zeros((h, w), dtype=np.float64)
    fallback = region & ~blk & ~node
    out[fallback] = (xs if view == "left" else -xs)[fallback]
    if nd:
        big = np.int64(1) << 62
        S = np.where((vol >= 0) & node[None], vol, big)
        j = nd - 1 - S[::-1].argmin(axis=0) if view == "left" else S.argmin(axis=0)
        d = (j + d0).astype(np.float64)
        if subpixel:
            def at(k):
                v = np.take_along_axis(S, np.clip(k, 0, nd - 1)[None], 0)[0]
                return np.where((k >= 0) & (k < nd), v, big)
            sm, s0, sp = at(j - 1), at(j), at(j + 1)
            ok = (sm < big) & (sp < big)
            num, den = np.where(ok, sm - sp, 0), np.where(ok, sm - 2 * s0 + sp, 0)
            ref = ok & (den > 0)
            q = num.astype(np.float64) / (2.0 * np.where(ref, den, 1).astype(np.float64))
            d = np.where(ref, ((j + d0).astype(np.float32) + q.astype(np.float32)).astype(np.float64), d)
        out[node] = d[node]
    return out


def search_np(L, R, view, block_size, min_disparity, max_disparity, cost, subpixel=False):
    """The census block-search map (float64; with subpixel the float32 values widened)."""
    return sgm_from_volume(volume(L, R, view, block_size, min_disparity, max_disparity, cost), view, 4, 0, 0, subpixel)


# ---- the literal restatement ------------------------------------------------------------------------------------------
def transform_py(img, cost):
    rx, ry = RADII[cost]
    h, w = img.shape[:2]
    Y = [[(1868 * int(img[y, x, 0]) + 9617 * int(img[y, x, 1]) + 4899 * int(img[y, x, 2]) + 8192) >> 14 for x in range(w)]
         for y in range(h)]
    T = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            k = 0
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    if dy == 0 and dx == 0:
                        continue
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and Y[yy][xx] < Y[y][x]:
                        T[y][x] |= 1 << k
                    k += 1
    return T


def _ham(a, b):
    v, n = a ^ b, 0
    while v:
        n += v & 1
        v >>= 1
    return n


def search_py(L, R, view, block_size, min_disparity, max_disparity, cost, subpixel=False):
    """The census block-search map, literally: one pixel, one candidate, one window pixel at a time."""
    TL, TR = transform_py(L, cost), transform_py(R, cost)
    h1, w1 = L.shape[:2]
    h2, w2 = R.shape[:2]
    rows = min(h1, h2)
    half = (block_size - 1) // 2
    h, w = (h1, w1) if view == "left" else (h2, w2)
    out = np.zeros((h, w), dtype=np.float64)
    for y in range(h):
        for x in range(w):
            c = {}
            if view == "left":
                if not (half <= y < rows - half and half <= x < w1 - half) or not L[y, x].any():
                    continue
                for d in range(1, max_disparity + 1):
                    cx = x - d
                    if cx < half:
                        break
                    if cx >= w2 - half:
                        continue
                    c[d] = sum(_ham(TL[y + dy][x + dx], TR[y + dy][cx + dx])
                               for dy in range(-half, half + 1) for dx in range(-half, half + 1))
            else:
                if y >= rows or not R[y, x].any():
                    continue
                left, right = min(x, half), min(w2 - x - 1, half)
                up, down = min(y, half), min(h2 - y - 1, half)
                if (left + right) * (up + down) > 0:
                    for d in range(min_disparity, max_disparity):
                        if x + d + right >= w1:
                            break
                        c[d] = sum(_ham(TL[yy][xx + d], TR[yy][xx]) for yy in range(y - up, y + down)
                                   for xx in range(x - left, x + right))
            if not c:
                out[y, x] = x if view == "left" else -x
                continue
            best = None
            for d in sorted(c):
                if best is None or c[d] < c[best] or (view == "left" and c[d] == c[best]):
                    best = d
            v = float(best)
            if subpixel and best - 1 in c and best + 1 in c:
                num = c[best - 1] - c[best + 1]
                den = c[best - 1] - 2 * c[best] + c[best + 1]
                if den > 0:
                    v = float(np.float32(best) + np.float32(num / (2.0 * den)))
            out[y, x] = v
    return out
