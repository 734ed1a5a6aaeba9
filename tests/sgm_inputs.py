"""Inputs for the device tests of semi-global matching at every register count (tests/test_gpu_sgm_forms.py), and the
table of the cases they run.  TEST INFRASTRUCTURE ONLY.

A path wave of ws_sgm.hip keeps disparity index j = 64 k + lane in register k of a lane, so the Lr(q, j +- 1) terms of
j = 64 k and 64 k - 1 cross from one register to the next at lanes 0 and 63.  A pair with one true disparity never
makes those terms decide a winner.  A staircase pair does: its true disparity climbs through the whole range, one step
at a time, so along every path the winner walks across every multiple of 64, and it is the P1 link between the two
sides of the multiple that lets it.  tests/test_sgm_inputs.py shows that on the CPU reference alone, for every case
of the table below.
"""
import zlib

import numpy as np


def staircase_disparity(w, h, lo, top, view):
    """d[y, x]: max(lo, 9 (x' - 8) // 10 + y % 3) clipped to top, x' = x in the left view and w - 1 - x in the right
    view (there x + d must stay inside the left image).  It moves by 0 or 1 per column and by 1, 1, -2 down the rows,
    so horizontal, vertical and diagonal paths all step."""
    yy, xx = np.mgrid[0:h, 0:w]
    if view == "right":
        xx = w - 1 - xx
    return np.clip(9 * (xx - 8) // 10 + yy % 3, lo, top)


def staircase_width(top, half):
    """The smallest width at which the staircase stands on its top step for eight columns inside the searched
    region: a little above top + 2 half + 8 by the staircase's slope of 9 / 10."""
    return (10 * top + 8) // 9 + 8 + half + 10


def staircase_pair(w, h, lo, top, seed, view="left", noise=3, levels=None):
    """A seeded pair of w x h images.  Left view: L[y, x] = R[y, x - d]; right view: R[y, x] = L[y, x + d], with
    d = staircase_disparity (source columns clipped to the image), plus independent noise on both images.  levels:
    few-level content without noise instead (ties between candidates)."""
    rng = np.random.default_rng(seed)
    if levels:
        src = (rng.integers(0, levels, size=(h, w, 3)) * (200 // max(1, levels - 1)) + 20).astype(np.int32)
        noise = 0
    else:
        src = rng.integers(1, 256, size=(h, w + 2, 3)).astype(np.int32)
        src = (src[:, :-2] + src[:, 1:-1] + src[:, 2:]) // 3
    d = staircase_disparity(w, h, lo, top, view)
    yy, xx = np.mgrid[0:h, 0:w]
    warped = src[yy, np.clip(xx - d if view == "left" else xx + d, 0, w - 1)]
    if noise:
        src = src + rng.integers(-noise, noise + 1, size=src.shape)
        warped = warped + rng.integers(-noise, noise + 1, size=warped.shape)
    src, warped = np.clip(src, 1, 255).astype(np.uint8), np.clip(warped, 1, 255).astype(np.uint8)
    return (warped, src) if view == "left" else (src, warped)


def nd_of(view, block_size, min_disparity, max_disparity, w1):
    """The number of disparities a search looks at (ws_ct.h: disparity_range), restated."""
    half = (block_size - 1) // 2
    if view == "left":
        return max(0, min(max_disparity, w1 - 1 - 2 * half))
    return 0 if max_disparity <= min_disparity else max(0, min(max_disparity, w1) - min_disparity)


def nj_of(nd):
    """The disparities per lane the path kernel is instantiated for (ws_sgm.hip: launch_paths_nj), restated."""
    per_lane = (nd + 63) // 64
    return next(n for n in (1, 2, 4, 8, 16, 32) if per_lane <= n)


# A P2 no path ever pays, so that winners move by single steps only and every step rests on a P1 link: just above
# the switch to 64-bit sums (paths (Cmax + P2) > 2^32 - 1) and just below it, for 8 and for 4 paths
BIG_P2 = {8: 600_000_000, 4: 1_100_000_000}
BIG_P2_32 = {8: 500_000_000, 4: 1_000_000_000}

# name: (view, cost, block_size, min_d, nd, h, paths, p1, p2, levels, (cost16, sum64))
STAIRCASES = {
    "129-left": ("left", "sad", 3, 0, 129, 4, 8, 20, 400, None, (1, 0)),
    "256-right": ("right", "ssd", 3, 0, 256, 4, 4, 50, BIG_P2[4], None, (0, 1)),
    "257-left": ("left", "ssd", 1, 0, 257, 6, 8, 50, 3000, None, (0, 0)),
    "512-right": ("right", "sad", 3, 2, 512, 5, 4, 20, BIG_P2[4], None, (1, 1)),
    "513-right": ("right", "ssd", 3, 0, 513, 4, 8, 300, BIG_P2_32[8], None, (0, 0)),
    "1024-left": ("left", "sad", 3, 0, 1024, 4, 8, 20, BIG_P2[8], None, (1, 1)),
    "1025-left": ("left", "ssd", 1, 0, 1025, 3, 4, 50, BIG_P2[4], None, (0, 1)),
    "1025-right": ("right", "sad", 3, 1, 1025, 3, 8, 20, BIG_P2[8], None, (1, 1)),
    "2048-left": ("left", "sad", 3, 0, 2048, 3, 4, 20, BIG_P2_32[4], None, (1, 0)),
    "2048-right": ("right", "ssd", 3, 0, 2048, 3, 4, 300, BIG_P2_32[4], None, (0, 0)),
    "600-left-levels": ("left", "ssd", 1, 0, 600, 6, 8, 50, 3000, 3, (0, 0)),
    "600-right-levels": ("right", "ssd", 3, 0, 601, 4, 4, 300, BIG_P2[4], 3, (0, 1)),
    # 364 x 72: three 32-row strips of the cost kernel, six 64-column tiles, five 64-disparity chunks under NJ = 8
    "seams-left": ("left", "sad", 3, 0, 310, 72, 8, 20, 400, None, (1, 0)),
}


def staircase_case(name):
    """(L, R, sgm_np's arguments, nd, (cost16, sum64)) of a case of STAIRCASES."""
    view, cost, bs, mind, nd, h, paths, p1, p2, levels, widths = STAIRCASES[name]
    half = (bs - 1) // 2
    lo = 1 if view == "left" else mind
    top = nd if view == "left" else mind + nd - 1
    maxd = nd if view == "left" else mind + nd
    w = staircase_width(top, half)
    seed = zlib.crc32(name.encode()) & 0xffff
    L, R = staircase_pair(w, h, lo, top, seed, view, levels=levels)
    assert nd_of(view, bs, mind, maxd, w) == nd
    return L, R, (view, bs, mind, maxd, cost, paths, p1, p2), nd, widths


# ---- image geometries the SGM calls accept and no seeded pair of the other files has --------------------------------
# name: (view, right image wider by (None: by max_disparity + 9, so that whole columns have no candidate), taller by,
# min_disparity).  The right view takes a right image at most one row taller (its windows would leave the left image).
GEOMETRIES = {
    "left-wider": ("left", 7, 0, 0),
    "left-taller": ("left", 0, 5, 0),
    "left-wider-taller": ("left", 9, 3, 0),
    "right-wider": ("right", None, 0, 0),
    "right-wider-min": ("right", None, 0, 2),
    "right-taller": ("right", 0, 1, 0),
    "right-taller-min": ("right", 0, 1, 3),
    "right-wider-taller-min": ("right", None, 1, 1),
}


def geometry_case(name, w1, h1, max_disparity):
    """(L, R, view, min_disparity) of a case of GEOMETRIES with a w1 x h1 left image: a shifted pair (true disparity
    max_disparity // 2) cut to the two sizes."""
    from test_subpixel_reference import shifted_pair
    view, dw, dh, mind = GEOMETRIES[name]
    w2 = w1 + (max_disparity + 9 if dw is None else dw)
    seed = zlib.crc32(name.encode()) & 0xffff
    L, R = shifted_pair(w1, h1 + dh, max_disparity // 2, seed, right_width=w2)
    return np.ascontiguousarray(L[:h1]), R, view, mind
