"""Two independent restatements of the uniqueness ratio and confidence rules of include/ws_stereo.h, for the tests.

TEST INFRASTRUCTURE ONLY.  Both work on the S that sgm_ref.volume (a census cost: census_cost_ref.volume) and
sgm_ref.aggregate give -- or, without sgm, on the window costs C themselves:
  * unique_from_sums: NumPy, int64 throughout.
  * unique_py: literal per-pixel, per-candidate loops in Python integers; the confidence goes through
    fractions.Fraction -> float -> np.float32.
Like `cut` in sgm_ref, the NumPy one takes two deliberately wrong variants (tests/test_unique_inputs.py only):
  rivals="all": every j != jb is a rival;  rivals="lanes": j = jb - 1, jb, jb + 1 (mod 64) are no rivals either -- what
  a winner kernel would compute that dropped a lane's whole offer instead of falling back to its runner-up.
"""
from fractions import Fraction

import numpy as np

import census_cost_ref
import sgm_ref
from sgm_ref import BIG


def volume(L, R, view, block_size, min_disparity, max_disparity, cost):
    """sgm_ref.volume, or for a census cost census_cost_ref.volume cut to the disparities the device looks at."""
    if cost.startswith("census"):
        return census_cost_ref.volume(L, R, view, block_size, min_disparity, max_disparity, cost)
    return sgm_ref.volume(L, R, view, block_size, min_disparity, max_disparity, cost)


def sums(V, sgm=None):
    """S [nd, h, w] int64, BIG where d is no candidate or the pixel no node.  sgm: None (S = C) or (paths, p1, p2)."""
    vol, d0, node, region, blk = V
    if sgm is None:
        return np.where((vol >= 0) & node[None], vol, BIG)
    paths, p1, p2 = sgm
    return sgm_ref.aggregate(vol, node, paths, p1, p2)[0]


def unique_from_sums(V, S, view, ratio, subpixel=False, rivals="rule"):
    """Rules 1-6 on S.  A dict: map (float64, the float32 values widened), conf (float32), counts (failed nodes, nodes),
    and per pixel jb, smin, m2 (BIG: uncontested), contested, fail."""
    vol, d0, node, region, blk = V
    nd = vol.shape[0]
    h, w = node.shape
    xs = np.broadcast_to(np.arange(w)[None, :], (h, w))
    out = np.zeros((h, w), dtype=np.float64)
    fallback = region & ~blk & ~node
    out[fallback] = (xs if view == "left" else -xs)[fallback]
    conf = np.zeros((h, w), dtype=np.float32)
    res = {"map": out, "conf": conf, "counts": (0, int(node.sum()))}
    if not nd:
        z = np.zeros((h, w), np.int64)
        res.update(jb=z, smin=z, m2=z + BIG, contested=node & False, fail=node & False)
        return res
    jb = nd - 1 - S[::-1].argmin(axis=0) if view == "left" else S.argmin(axis=0)   # rule 1, the view's tie rule
    smin = np.take_along_axis(S, jb[None], 0)[0]
    idx = np.arange(nd)[:, None, None]
    if rivals == "all":
        rival = idx != jb[None]
    else:
        rival = np.abs(idx - jb[None]) >= 2                                           # rule 2
        if rivals == "lanes":
            rival &= (idx - jb[None] + 1) % 64 > 2
        else:
            assert rivals == "rule"
    m2 = np.where(rival & (S < BIG), S, BIG).min(axis=0)
    contested = node & (m2 < BIG)
    a = np.where(contested, m2, 0) * (100 - ratio)
    b = np.where(contested, smin, 0) * 100
    fail = contested & (a < b)                                                        # rule 3
    d = (jb + d0).astype(np.float64)
    if subpixel:
        def at(k):
            v = np.take_along_axis(S, np.clip(k, 0, nd - 1)[None], 0)[0]
            return np.where((k >= 0) & (k < nd), v, BIG)
        sm, s0, sp = at(jb - 1), at(jb), at(jb + 1)
        ok = (sm < BIG) & (sp < BIG)
        num, den = np.where(ok, sm - sp, 0), np.where(ok, sm - 2 * s0 + sp, 0)
        ref = ok & (den > 0)
        q = num.astype(np.float64) / (2.0 * np.where(ref, den, 1).astype(np.float64))
        d = np.where(ref, ((jb + d0).astype(np.float32) + q.astype(np.float32)).astype(np.float64), d)
    out[node] = d[node]
    out[fail] = 0.0                                                                   # rule 4
    pos = contested & (m2 > 0)                                                        # rule 5
    quo = (np.where(pos, m2 - smin, 0).astype(np.float64) / np.where(pos, m2, 1).astype(np.float64)).astype(np.float32)
    conf[node] = 1.0
    conf[contested] = 0.0
    conf[pos] = quo[pos]
    res.update(counts=(int(fail.sum()), int(node.sum())), jb=jb, smin=smin, m2=m2, contested=contested, fail=fail)
    return res


def unique_np(L, R, view, block_size, min_disparity, max_disparity, cost, ratio, sgm=None, subpixel=False, rivals="rule"):
    V = volume(L, R, view, block_size, min_disparity, max_disparity, cost)
    return unique_from_sums(V, sums(V, sgm), view, ratio, subpixel, rivals)


def unique_py(V, S, view, ratio, subpixel=False):
    """The literal restatement: (map float64, conf float32, (failed nodes, nodes))."""
    vol, d0, node, region, blk = V
    nd = vol.shape[0]
    h, w = node.shape
    out = np.zeros((h, w), dtype=np.float64)
    conf = np.zeros((h, w), dtype=np.float32)
    failed = nodes = 0
    for y in range(h):
        for x in range(w):
            if not node[y, x]:
                if region[y, x] and not blk[y, x]:
                    out[y, x] = x if view == "left" else -x
                continue
            nodes += 1
            s = {j: int(S[j, y, x]) for j in range(nd) if vol[j, y, x] >= 0}
            best = None
            for j in sorted(s):
                if best is None or s[j] < s[best] or (view == "left" and s[j] == s[best]):
                    best = j
            v = float(d0 + best)
            if subpixel and best - 1 in s and best + 1 in s:
                num = s[best - 1] - s[best + 1]
                den = s[best - 1] - 2 * s[best] + s[best + 1]
                if den > 0:
                    v = float(np.float32(d0 + best) + np.float32(num / (2.0 * den)))
            rivals = [s[j] for j in s if abs(j - best) >= 2]
            if not rivals:
                conf[y, x] = 1.0
            else:
                m2 = min(rivals)
                conf[y, x] = np.float32(float(Fraction(m2 - s[best], m2))) if m2 > 0 else 0.0
                if m2 * (100 - ratio) < s[best] * 100:
                    v = 0.0
                    failed += 1
            out[y, x] = v
    return out, conf, (failed, nodes)
