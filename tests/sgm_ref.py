"""Two independent restatements of the semi-global matching rules of include/ws_stereo.h, for the tests.

TEST INFRASTRUCTURE ONLY.
  * sgm_np: NumPy, int64 throughout.  The window costs are the block search's own cost volumes
    (oracle/brute.py:cost_volume_left, tests/test_subpixel_reference.py:cost_volume_right); each path is walked one
    step at a time, vectorised across a whole image row or column per step.
  * sgm_py: literal per-pixel loops in plain Python integers for tiny images: its own windows, its own candidate
    sets, one pixel and one disparity at a time.
Both return the map as float64 (integer-valued) or, with subpixel, the float32 values widened to float64.
"""
import numpy as np

from oracle import brute
from test_subpixel_reference import cost_volume_right

BIG = np.int64(1) << 62
DIRS4 = [(1, 0), (-1, 0), (0, 1), (0, -1)]
DIRS8 = DIRS4 + [(1, 1), (-1, -1), (-1, 1), (1, -1)]


def _black(img):
    return (img == 0).all(axis=2)


def volume(L, R, view, block_size, min_disparity, max_disparity, cost):
    """(vol [nd, h, w] int64 with -1 where d is no candidate, d0, node mask, region mask, black mask) of the view's map."""
    h1, w1 = L.shape[:2]
    h2, w2 = R.shape[:2]
    rows = min(h1, h2)
    half = (block_size - 1) // 2
    if view == "left":
        nd = max(0, max_disparity)
        vol = brute.cost_volume_left(L, R, block_size, nd, cost) if nd else np.zeros((0, h1, w1), np.int64)
        d0, h, w = 1, h1, w1
        region = np.zeros((h1, w1), bool)
        region[half:rows - half, half:w1 - half] = True
        blk = _black(L)
    else:
        if max_disparity > min_disparity:
            vol = cost_volume_right(L, R, block_size, min_disparity, max_disparity, cost)
        else:
            vol = np.zeros((0, h2, w2), np.int64)
        d0, h, w = min_disparity, h2, w2
        region = np.zeros((h2, w2), bool)
        region[:rows] = True
        blk = _black(R)
    valid = vol >= 0
    node = region & ~blk & valid.any(axis=0) if vol.shape[0] else np.zeros((h, w), bool)
    return vol, d0, node, region, blk


def _step(Lq, vq, qnode, C, vp, p1, p2, cut=None):
    """One path step across a line of pixels: Lq, vq, C, vp are [nd, n]; qnode [n].  Returns Lr [nd, n] (BIG where d is
    not a candidate of p).  cut (tests/test_sgm_inputs.py only): indices j whose P1 link with j - 1 is left out, in both
    directions -- a deliberately wrong aggregation that shows which pixels of a map the link decides."""
    lq = np.where(vq, Lq, BIG)
    m = lq.min(axis=0) if lq.shape[0] else np.zeros(lq.shape[1], np.int64)
    best = np.minimum(lq, m[None, :] + p2)
    if lq.shape[0] > 1:
        dn, up = vq[:-1], vq[1:]
        if cut is not None:
            link = np.ones(lq.shape[0] - 1, bool)
            link[np.asarray(cut, dtype=np.int64) - 1] = False
            dn, up = dn & link[:, None], up & link[:, None]
        best[1:] = np.minimum(best[1:], np.where(dn, Lq[:-1] + p1, BIG))   # Lr(q, d-1) + P1
        best[:-1] = np.minimum(best[:-1], np.where(up, Lq[1:] + p1, BIG))   # Lr(q, d+1) + P1
    lr = C + np.where(qnode[None, :], best - m[None, :], 0)
    return np.where(vp, lr, BIG)


def path_costs(vol, node, r, p1, p2, cut=None):
    """Lr for direction r = (dx, dy): [nd, h, w] int64, BIG where d is no candidate or the pixel no node."""
    nd, h, w = vol.shape
    dx, dy = r
    valid = (vol >= 0) & node[None]
    C = np.where(valid, vol, 0)
    out = np.full(vol.shape, BIG, dtype=np.int64)
    if dy == 0:   # walk the columns, all rows at once
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        prev = None
        for x in xs:
            if prev is None:
                lr = np.where(valid[:, :, x], C[:, :, x], BIG)
            else:
                lr = _step(out[:, :, prev], valid[:, :, prev], node[:, prev], C[:, :, x], valid[:, :, x], p1, p2, cut)
            out[:, :, x] = lr
            prev = x
        return out
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    prev = None
    for y in ys:
        if prev is None:
            out[:, y, :] = np.where(valid[:, y, :], C[:, y, :], BIG)
        else:
            # predecessor column x - dx on row prev; outside the image: a restart
            xq = np.arange(w) - dx
            inside = (xq >= 0) & (xq < w)
            xqc = np.clip(xq, 0, w - 1)
            Lq = out[:, prev, xqc]
            vq = valid[:, prev, xqc] & inside[None]
            qn = node[prev, xqc] & inside
            out[:, y, :] = _step(Lq, vq, qn, C[:, y, :], valid[:, y, :], p1, p2, cut)
        prev = y
    return out


def aggregate(vol, node, paths, p1, p2, cut=None):
    """S [nd, h, w] int64 (BIG where d is no candidate or the pixel no node) and the largest Lr met."""
    S = np.zeros(vol.shape, dtype=np.int64)
    valid = (vol >= 0) & node[None]
    lmax = 0
    for r in (DIRS4 if paths == 4 else DIRS8):
        lr = path_costs(vol, node, r, p1, p2, cut)
        if valid.any():
            lmax = max(lmax, int(lr[valid].max()))
        S += np.where(valid, lr, 0)
    return np.where(valid, S, BIG), lmax


def sgm_np(L, R, view, block_size, min_disparity, max_disparity, cost="ssd", paths=8, p1=0, p2=0, subpixel=False,
           return_lmax=False, cut=None):
    """The map of an SGM search (float64; with subpixel the float32 values widened).  cut: see _step; None is the rule."""
    V = volume(L, R, view, block_size, min_disparity, max_disparity, cost)
    return sgm_from_volume(V, view, paths, p1, p2, subpixel, return_lmax, cut)


def sgm_from_volume(V, view, paths=8, p1=0, p2=0, subpixel=False, return_lmax=False, cut=None):
    """sgm_np on what volume() returned (left unchanged), for callers that aggregate the same costs more than once."""
    vol, d0, node, region, blk = V
    nd = vol.shape[0]
    h, w = node.shape
    S, lmax = aggregate(vol, node, paths, p1, p2, cut)
    xs = np.broadcast_to(np.arange(w)[None, :], (h, w))
    out = np.zeros((h, w), dtype=np.float64)
    fallback = region & ~blk & ~node
    out[fallback] = (xs if view == "left" else -xs)[fallback]
    if nd:
        j = nd - 1 - S[::-1].argmin(axis=0) if view == "left" else S.argmin(axis=0)   # tie rule
        d = (j + d0).astype(np.float64)
        if subpixel:
            def at(k):
                kk = np.clip(k, 0, nd - 1)
                v = np.take_along_axis(S, kk[None], 0)[0]
                return np.where((k >= 0) & (k < nd), v, BIG)
            sm, s0, sp = at(j - 1), at(j), at(j + 1)
            ok = (sm < BIG) & (sp < BIG)
            num = np.where(ok, sm - sp, 0)
            den = np.where(ok, sm - 2 * s0 + sp, 0)
            ref = ok & (den > 0)
            q = num.astype(np.float64) / (2.0 * np.where(ref, den, 1).astype(np.float64))
            d = np.where(ref, ((j + d0).astype(np.float32) + q.astype(np.float32)).astype(np.float64), d)
        out[node] = d[node]
    return (out, lmax) if return_lmax else out


# ---- the literal restatement ------------------------------------------------------------------------------------------
def _pc(a, b, cost):
    s = 0
    for c in range(3):
        t = int(a[c]) - int(b[c])
        s += abs(t) if cost == "sad" else t * t
    return s


def _candidates_py(L, R, view, block_size, min_disparity, max_disparity, cost, y, x):
    """{d: C(p, d)} of pixel (y, x) of the view's map, or None if the pixel is outside the searched region / black."""
    h1, w1 = L.shape[:2]
    h2, w2 = R.shape[:2]
    rows = min(h1, h2)
    half = (block_size - 1) // 2
    out = {}
    if view == "left":
        if not (half <= y < rows - half and half <= x < w1 - half) or not L[y, x].any():
            return None
        for d in range(1, max_disparity + 1):
            cx = x - d
            if cx < half or cx >= w2 - half:
                continue
            out[d] = sum(_pc(L[y + dy, x + dx], R[y + dy, cx + dx], cost)
                         for dy in range(-half, half + 1) for dx in range(-half, half + 1))
        return out
    if y >= rows or not R[y, x].any():
        return None
    left, right = min(x, half), min(w2 - x - 1, half)
    up, down = min(y, half), min(h2 - y - 1, half)
    if (left + right) * (up + down) == 0:
        return out
    for d in range(min_disparity, max_disparity):
        if x + d + right >= w1:
            break
        out[d] = sum(_pc(L[yy, xx + d], R[yy, xx], cost) for yy in range(y - up, y + down) for xx in range(x - left, x + right))
    return out


def sgm_py(L, R, view, block_size, min_disparity, max_disparity, cost="ssd", paths=8, p1=0, p2=0, subpixel=False):
    h, w = (L if view == "left" else R).shape[:2]
    K = {}
    fallback = set()
    for y in range(h):
        for x in range(w):
            c = _candidates_py(L, R, view, block_size, min_disparity, max_disparity, cost, y, x)
            if c:
                K[(y, x)] = c
            elif c is not None:
                fallback.add((y, x))
    S = {p: {d: 0 for d in c} for p, c in K.items()}
    for dx, dy in (DIRS4 if paths == 4 else DIRS8):
        Lr = {}
        ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
        xs = list(range(w)) if dx >= 0 else list(range(w - 1, -1, -1))
        for y in ys:
            for x in xs:
                if (y, x) not in K:
                    continue
                q = (y - dy, x - dx)
                here = {}
                for d, c in K[(y, x)].items():
                    if q not in K:
                        here[d] = c
                        continue
                    lq = Lr[q]
                    m = min(lq.values())
                    terms = [m + p2]
                    if d in lq:
                        terms.append(lq[d])
                    if d - 1 in lq:
                        terms.append(lq[d - 1] + p1)
                    if d + 1 in lq:
                        terms.append(lq[d + 1] + p1)
                    here[d] = c + min(terms) - m
                Lr[(y, x)] = here
                for d, v in here.items():
                    S[(y, x)][d] += v
    out = np.zeros((h, w), dtype=np.float64)
    for (y, x) in fallback:
        out[y, x] = x if view == "left" else -x
    for (y, x), s in S.items():
        best = None
        for d in sorted(s):
            if best is None or s[d] < s[best] or (view == "left" and s[d] == s[best]):
                best = d
        v = float(best)
        if subpixel and best - 1 in s and best + 1 in s:
            num = s[best - 1] - s[best + 1]
            den = s[best - 1] - 2 * s[best] + s[best + 1]
            if den > 0:
                v = float(np.float32(best) + np.float32(num / (2.0 * den)))
        out[y, x] = v
    return out
