"""Stereo pairs built for the matrix-core SSD kernel (csrc/ws_march_mfma.h), plain NumPy.

The kernel keeps a candidate (x, d) in one accumulator register: with e = d - 1 = 32 (8 - t) + n - m it is tile t,
row m of the tile (register i and lane half h: m = (i & 3) + 8 (i >> 2) + 4 h), lane column n = (x - 3) % 32, x-wave
wx = ((x - 3) % 128) // 32 and d-wave wv = t // 5.  Each register has a bias word, a tie tag and a poison of its own,
and a wrong one shows only where that register wins.  The pairs below make chosen candidates win:

  * disparity_ladder: row bands of one true disparity each, exact copies, so that every (d, column of the tile) wins;
  * tie_ladder: row bands periodic along x, so that every multiple of the period ties at cost 0 and only the tie rules
    (tags inside a tile, strict '<' between tiles, the exchange between lane halves, the merge of the two d-waves
    through LDS) decide.

tests/test_mfma_inputs.py holds the conditions these pairs meet, checked on the CPU reference alone.
"""
import numpy as np

BS = 7
HALF = 3
TILE_COLS = 128        # columns of one workgroup's tile: 4 x-waves of 32 lanes


def disparity_ladder(w, band, seed, ds):
    """(left, right): len(ds) bands of `band` rows; left is i.i.d. bytes in [1, 255] (never black), right independent
    noise with right[y, :w - d] = left[y, d:] inside the band of d."""
    ds = [int(d) for d in ds]
    rng = np.random.default_rng(seed)
    h = band * len(ds)
    left = rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8)
    right = rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8)
    for k, d in enumerate(ds):
        if 0 < d < w:
            right[k * band:(k + 1) * band, :w - d] = left[k * band:(k + 1) * band, d:]
    return left, right


def tie_ladder(w, band, periods, seed):
    """(left, right), right == left: one band of `band` rows per period p, each row noise of period p along x."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in periods:
        cell = rng.integers(1, 256, size=(band, int(p), 3), dtype=np.uint8)
        rows.append(np.tile(cell, (1, -(-w // int(p)), 1))[:, :w])
    left = np.concatenate(rows, axis=0)
    return left, left.copy()


SWEEP_DS = (1, 2, 33, 34, 65, 66, 97, 98, 129, 130, 161, 162, 193, 194, 225, 226, 256, 255, 128, 160, 32, 100)


def range_sweep_pair(w, h, seed=23, band=9):
    """The one pair every max_disparity is searched on: a ladder of the disparities around the steps of the kernel's
    `active` mask, cropped to h rows.  A band whose d lies beyond the range searched is noise against noise there, where
    every candidate inside the range wins somewhere; a few black pixels on each side."""
    n = -(-h // band)
    ds = [SWEEP_DS[k % len(SWEEP_DS)] for k in range(n)]
    left, right = disparity_ladder(w, band, seed, ds)
    left, right = left[:h].copy(), right[:h].copy()
    left[h // 2, w // 3:w // 3 + 5] = 0
    right[h // 3, w // 2:w // 2 + 5] = 0
    return left, right


def clean_rows(band, k):
    """The rows of band k whose 7 window rows all lie inside the band."""
    return range(k * band + HALF, (k + 1) * band - HALF)


def ladder_expected(w, band, ds, maxd):
    """[(row, first column, expected disparity)] for every clean row of every band whose d is a candidate: the map
    equals d from column d + 3 to the interior's end."""
    return [(y, d + HALF, d) for k, d in enumerate(ds) if 1 <= d <= maxd and d + HALF < w - HALF for y in clean_rows(band, k)]


def tie_expected_row(w, p, maxd):
    """(first column, values): on a clean row of period p the largest multiple of p among the candidates wins,
    p * (min(D, x - 3) // p), for x >= p + 3."""
    x = np.arange(p + HALF, w - HALF)
    return p + HALF, (p * (np.minimum(maxd, x - HALF) // p)).astype(np.float64)


def census(disparity_map, maxd=256):
    """cells[d - 1, c]: candidate d won at a pixel of tile column c = (x - 3) % 128 somewhere in the interior."""
    h, w = disparity_map.shape
    cells = np.zeros((maxd, TILE_COLS), dtype=bool)
    inner = disparity_map[HALF:h - HALF, HALF:w - HALF]
    col = np.broadcast_to((np.arange(HALF, w - HALF) - HALF) % TILE_COLS, inner.shape)
    d = inner.astype(np.int64)
    ok = (d >= 1) & (d <= maxd) & (inner == d)
    cells[d[ok] - 1, col[ok]] = True
    return cells


def slot_of(d, x):
    """(t, i, h, n, wx, wv) of candidate d at column x for a search with d_lo = 1.  Diagnostic only: a restatement of
    the kernel's register map, checked for nothing but self-consistency, used to NAME the register behind a missing
    census cell in a failure message.  No assertion about the kernel rests on it: the census counts (d, tile column)
    cells of the map, which are defined without it."""
    c = (x - HALF) % TILE_COLS
    n, wx = c % 32, c // 32
    e = d - 1
    t = 8 - (e - n + 31) // 32
    m = 32 * (8 - t) + n - e
    h, r = (m >> 2) & 1, m & 3
    i = r + 4 * (m >> 3)
    return t, i, h, n, wx, t // 5


TIE_PERIODS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 96, 128, 159, 160, 161, 255)
