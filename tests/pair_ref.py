"""Two independent restatements of "both views from one volume" (include/ws_stereo.h), for the tests.

TEST INFRASTRUCTURE ONLY.  Both work on the S of the base view that unique_ref.sums gives (BIG where d is no candidate
of the base pixel or the pixel is no node):
  * derived_np: NumPy, a scatter-minimum per disparity -- every base column offers S(., d) to the derived column
    x - d (base left) or x + d (base right).
  * derived_py: literal -- for each derived pixel, its candidates gathered in Python integers.
derived_np takes a deliberately wrong tie="other" (the other view's tie rule) for tests/test_pair_inputs.py.
pair_np strings the base map (unique_ref), the derived map and the check (lr_ref) together as the pair call does.
"""
import numpy as np

import lr_ref
from sgm_ref import BIG
from unique_ref import sums, unique_from_sums, volume


def other_shape(L, R, view):
    """The derived map's (h, w): the other view's image."""
    return (R if view == "left" else L).shape[:2]


def derived_np(S, d0, view, shape, tie="rule", winners=False):
    """The derived map (float64, integer-valued) of base view `view` on a map of `shape`.  winners: also the winning
    disparity index j per derived pixel (-1: no candidate)."""
    nd, h, w = S.shape
    ho, wo = shape
    rows = min(h, ho)
    smallest = (view == "left") == (tie == "rule")   # base left: the smallest d wins
    assert tie in ("rule", "other")
    best = np.full((ho, wo), BIG, dtype=np.int64)
    jb = np.full((ho, wo), -1, dtype=np.int64)
    xs = np.arange(w)
    for j in range(nd):
        d = d0 + j
        c = xs - d if view == "left" else xs + d
        ok = (c >= 0) & (c < wo)
        s = S[j, :rows][:, ok]
        cur = best[:rows, c[ok]]
        upd = (s < cur) if smallest else ((s <= cur) & (s < BIG))   # j ascends: a later equal one is the larger d
        best[:rows, c[ok]] = np.where(upd, s, cur)
        jb[:rows, c[ok]] = np.where(upd, j, jb[:rows, c[ok]])
    out = np.where(jb >= 0, jb + d0, 0).astype(np.float64)
    return (out, jb) if winners else out


def derived_py(S, d0, view, shape):
    """The literal restatement."""
    nd, h, w = S.shape
    ho, wo = shape
    out = np.zeros((ho, wo), dtype=np.float64)
    for y in range(min(h, ho)):
        for xo in range(wo):
            cand = []
            for j in range(nd):
                d = d0 + j
                x = xo + d if view == "left" else xo - d
                if 0 <= x < w and int(S[j, y, x]) < int(BIG):
                    cand.append((int(S[j, y, x]), d))
            if cand:
                smin = min(s for s, _ in cand)
                ds = [d for s, d in cand if s == smin]
                out[y, xo] = float(min(ds) if view == "left" else max(ds))
    return out


def pair_np(L, R, view, block_size, min_disparity, max_disparity, cost, sgm=None, ratio=None, subpixel=False, lr=None,
            tie="rule"):
    """A dict: left, right (the raw maps, float64), unique_counts (base winner's, ratio None: at ratio 0) and, with
    lr = (max_diff, fill), checked_left, checked_right (float32) and lr_counts."""
    V = volume(L, R, view, block_size, min_disparity, max_disparity, cost)
    S = sums(V, sgm)
    base = unique_from_sums(V, S, view, 0 if ratio is None else ratio, subpixel)
    der = derived_np(S, V[1], view, other_shape(L, R, view), tie)
    res = {"left": base["map"] if view == "left" else der, "right": der if view == "left" else base["map"],
           "unique_counts": base["counts"]}
    if lr is not None:
        cl, cr, counts = lr_ref.lr_check(res["left"].astype(np.float32), res["right"].astype(np.float32), lr[0], lr[1])
        res.update(checked_left=cl, checked_right=cr, lr_counts=counts)
    return res
