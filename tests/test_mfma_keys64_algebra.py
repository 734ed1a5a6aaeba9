"""The packed key of the matrix-core SSD kernel (csrc/ws_march_mfma.h), modelled on uint64 pairs in NumPy: no device.

The kernel forms the keys of accumulator registers 2q and 2q + 1 with ONE 64-bit shift-and-add, (pair << 4) + bias pair.
That is two independent 32-bit keys only if nothing crosses from the low word into the high one, which the header
arranges with uniform offsets (kMfmaA0, kMfmaG0), poisons that obey the same bounds, and a bound on the rows a strip
enters (kMfmaMaxSteps).  The constants are read from the header, so this file follows them; the ranges are restated
here from the window's geometry and not taken from the header's asserts:

  centred bytes in [-128, 127], K = 21 bytes per window row, WH = 7 rows, N = kMfmaMaxSteps rows entered:
    cross = sum a^ b^ over the window, T = sum b^ over a window row, E = sum of T over the rows entered,
    Acc = A0 (+ PA) - cross - E,   gsum = G0 (+ PG) + (window sum of b^^2) + 2 E,   bias' = gsum << 3 | q,
    key = (Acc << 4) + bias' = (C0 + cost (+ 2 PA) (+ PG)) << 3 | q,   cost = sum b^^2 - 2 cross.

The second half checks the two-chain minimum (low words, high words), the tile-level chain and the decode against a
plain argmin under the kernel's tie rule: smaller G = 32 t + m on equal cost, m = (i & 3) + 8 (i >> 2) + 4 h.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stereo_reconstruction_amd", "csrc", "ws_march_mfma.h")

K, WH = 21, 7
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _constants():
    text = open(HEADER).read()

    def shift(name):
        m = re.search(r"\b%s = 1LL << (\d+)" % name, text)
        assert m, name
        return 1 << int(m.group(1))

    c = {n: shift(n) for n in ("kMfmaA0", "kMfmaAccPoison", "kMfmaG0", "kMfmaBiasPoison")}
    c["steps"] = int(re.search(r"kMfmaMaxSteps = (\d+);", text).group(1))
    c["kt"] = int(re.search(r"kMfmaKT = (\d+);", text).group(1))
    m = re.search(r"kMfmaValidBound = kMfmaC0 \+ \(1LL << (\d+)\)", text)
    c["C0"] = 2 * c["kMfmaA0"] + c["kMfmaG0"]
    c["valid"] = c["C0"] + (1 << int(m.group(1)))
    return c


C = _constants()
A0, PA, G0, PG, N, KT, C0, VALID = (C["kMfmaA0"], C["kMfmaAccPoison"], C["kMfmaG0"], C["kMfmaBiasPoison"], C["steps"], C["kt"],
                                    C["C0"], C["valid"])


def pack(lo, hi):
    return (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)


def lshl_add_u64(a, b):
    """v_lshl_add_u64 with a shift of 4: (a << 4) + b modulo 2^64, on uint64 arrays."""
    return (a << np.uint64(4)) + b          # NumPy's uint64 arithmetic wraps, as the instruction does


def keys_of(acc, gsum, q):
    """acc, gsum: int64 arrays (..., 2) holding the two registers of a pair WITH their offsets and poisons; q: the pair's
    index.  Returns (lo key, hi key) as the kernel computes them, after asserting the conditions of the packed add."""
    acc, gsum = np.asarray(acc, dtype=np.int64), np.asarray(gsum, dtype=np.int64)
    assert (acc >= 0).all() and (acc < (1 << 28)).all(), "the top 4 bits of a shifted word are zero"
    bias = (gsum << KT) | q
    assert (gsum >= 0).all() and (bias < (1 << 31)).all(), "a bias word is a non-negative int"
    exact = (acc << 4) + bias                  # the two 32-bit keys, computed apart in int64
    assert (exact <= M32).all(), "no carry leaves the low word and no key wraps"
    k = lshl_add_u64(pack(acc[..., 0], acc[..., 1]), pack(bias[..., 0], bias[..., 1]))
    lo, hi = (k & np.uint64(M32)).astype(np.int64), (k >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(lo, exact[..., 0]) and np.array_equal(hi, exact[..., 1]), "the packed add is the two 32-bit adds"
    return lo, hi


def test_constants_are_the_key_form():
    assert KT == 3 and C0 == 2 * A0 + G0
    assert N >= 2160 + WH - 1, "above every strip of the plan census's tallest image"


def _extremes():
    """(cross, E, sumsq) at the limits of their ranges after N rows entered."""
    out = []
    for b in (-128, 127):                      # all-dark and all-bright target rows
        e, sq = b * K * N, b * b * K * WH
        for a in (-128, 127):                  # a left image of either extreme
            out.append((a * b * K * WH, e, sq))
    return out


@pytest.mark.parametrize("pa", (0, 1))
@pytest.mark.parametrize("pg", (0, 1))
def test_ranges_at_the_step_bound(pa, pg):
    rng = np.random.default_rng(5 + 2 * pa + pg)
    xb, eb = 128 * 128 * K * WH, 128 * K * N
    n = 4096
    cross = rng.integers(-128 * 127 * K * WH, xb + 1, size=(n, 2))
    e = rng.integers(-eb, 127 * K * N + 1, size=(n, 2))
    sq = rng.integers(0, xb + 1, size=(n, 2))
    ext = np.array(_extremes(), dtype=np.int64)
    # every extreme in both words of a pair, and every extreme next to every other
    pairs = np.array([(x, y) for x in ext for y in ext], dtype=np.int64)             # (16, 2, 3)
    cross = np.concatenate([cross, pairs[:, :, 0]])
    e = np.concatenate([e, pairs[:, :, 1]])
    sq = np.concatenate([sq, pairs[:, :, 2]])
    acc = A0 + pa * PA - cross - e
    gsum = G0 + pg * PG + sq + 2 * e
    for q in (0, (1 << KT) - 1):
        lo, hi = keys_of(acc, gsum, q)
        cost = sq - 2 * cross
        want = ((C0 + cost + 2 * pa * PA + pg * PG) << KT) | q
        assert np.array_equal(lo, want[:, 0]) and np.array_equal(hi, want[:, 1])
        cw = np.stack([lo, hi], axis=-1) >> KT
        if pa or pg:
            assert (cw >= VALID).all(), "a poisoned cost word is at or above the bound"
        else:
            assert (cw < VALID).all() and (cw >= 0).all(), "a valid cost word is below it"


def test_every_poisoned_key_is_above_every_valid_key():
    lo_cost, hi_cost = -2 * 128 * 128 * K * WH, 128 * 128 * K * WH + 2 * 128 * 127 * K * WH
    top_valid = ((C0 + hi_cost) << KT) | ((1 << KT) - 1)
    for extra in (2 * PA, PG, 2 * PA + PG):
        assert ((C0 + lo_cost + extra) << KT) > top_valid
        assert ((C0 + hi_cost + extra) << KT) | ((1 << KT) - 1) <= M32
    assert (top_valid >> KT) < VALID <= C0 + lo_cost + min(2 * PA, PG)


# ---- the winner ---------------------------------------------------------------------------------------------------------

def row_of(i, h):
    return (i & 3) + 8 * (i >> 2) + 4 * h


def kernel_winner(cost, h, rng):
    """cost: int64 (tiles, 16) true cost words of one lane half (poisons included by the caller as large costs).
    Models mfma_tile_best / mfma_best_code and the decode in front of mfma_pair_best; returns (cost word, G)."""
    tiles = cost.shape[0]
    best_k = best_l = M32
    best_t = 0
    for t in range(tiles):
        # split each cost word into an accumulator and a bias sum at random: only their sum is the key
        e = rng.integers(-128 * K * N, 127 * K * N + 1, size=(8, 2))
        c = cost[t].reshape(8, 2)
        gs = (c & 1) + 2 * rng.integers(0, 1000, size=(8, 2)) + 2 * e      # gsum's parity is the cost's
        ac = (c - gs) // 2                                                 # 2 Acc + gsum = cost
        lo, hi = keys_of(A0 + ac, G0 + gs, np.arange(8)[:, None].repeat(2, axis=1))
        kl, kh = min(lo[0], lo[1]), min(hi[0], hi[1])
        for q in range(2, 8, 2):
            kl, kh = min(min(kl, lo[q]), lo[q + 1]), min(min(kh, hi[q]), hi[q + 1])
        km = min(kl, kh)
        if t == 0 or (km | ((1 << KT) - 1)) < best_k:
            best_k, best_l, best_t = km, kl, t
    code = 2 * best_t + (1 if best_k < best_l else 0)
    i = 2 * (best_k & ((1 << KT) - 1)) + (code & 1)
    return (best_k >> KT) - C0, 32 * (code >> 1) + row_of(i, h)


def reference_winner(cost, h):
    cands = sorted((int(cost[t, i]), 32 * t + row_of(i, h)) for t in range(cost.shape[0]) for i in range(16))
    return cands[0]


def _tie_cases():
    big = 5000
    cases = []

    def base():
        return np.full((5, 16), big, dtype=np.int64) + np.arange(80).reshape(5, 16)

    def tie(name, cells, value=-7):
        c = base()
        for t, i in cells:
            c[t, i] = value
        cases.append((name, c))

    for q in range(8):
        tie("within_pair_%d" % q, [(2, 2 * q), (2, 2 * q + 1)])
    tie("between_pairs_L", [(1, 4), (1, 10)])
    tie("between_pairs_H", [(1, 5), (1, 11)])
    tie("between_pairs_all", [(3, i) for i in range(16)])
    tie("L_H_qH_below_qL", [(2, 2 * 5), (2, 2 * 2 + 1)])
    tie("L_H_qH_equal_qL", [(2, 2 * 4), (2, 2 * 4 + 1)])
    tie("L_H_qH_above_qL", [(2, 2 * 1), (2, 2 * 6 + 1)])
    tie("between_tiles_L_then_H", [(1, 6), (3, 1)])
    tie("between_tiles_H_then_L", [(1, 7), (3, 0)])
    tie("between_tiles_first", [(0, 15), (4, 0)])
    tie("every_cell", [(t, i) for t in range(5) for i in range(16)])
    tie("negative_limit", [(4, 9), (4, 3)], value=-2 * 128 * 128 * K * WH)
    tie("positive_limit", [(t, i) for t in range(5) for i in range(16) if (t, i) != (3, 13)], value=3 * 128 * 128 * K * WH)
    # a tile whose best is poisoned: it never beats a valid one, and among poisoned ones the rule is the same
    c = base()
    c[0] += 2 * PA
    c[1] += PG
    c[2, 9] = c[3, 9] = 11
    cases.append(("poisoned_tiles", c))
    cases.append(("all_poisoned", base() + 2 * PA + PG))
    return cases


@pytest.mark.parametrize("h", (0, 1))
@pytest.mark.parametrize("case", [c for _, c in _tie_cases()], ids=[n for n, _ in _tie_cases()])
def test_two_chain_winner_on_ties(case, h):
    rng = np.random.default_rng(17 + h)
    assert kernel_winner(case, h, rng) == reference_winner(case, h)


def test_two_chain_winner_on_random_costs():
    rng = np.random.default_rng(99)
    for trial in range(200):
        tiles = int(rng.integers(1, 6))
        cost = rng.integers(-20, 20, size=(tiles, 16))          # a narrow range: ties everywhere
        if trial % 3 == 0:
            cost = cost + (rng.integers(0, 2, size=(tiles, 16)) * 2 * PA) + (rng.integers(0, 2, size=(tiles, 16)) * PG)
        for h in (0, 1):
            assert kernel_winner(cost, h, rng) == reference_winner(cost, h), (trial, h)


# ---- the launcher's side of the bound -----------------------------------------------------------------------------------

_PLAN_CHILD = r"""
import json
import sys
sys.path.insert(0, %r)
import stereo_reconstruction_amd as ws
p = ws.make_params(ws.VIEW_LEFT, 7, 0, 256, 1.0, "ssd")
print(json.dumps([ws.plan(p, (h, 400, 3), (h, 400, 3)) for h in json.loads(sys.argv[1])]))
"""


def test_plan_refuses_strips_beyond_the_bound(wslib):
    """One strip per image (WS_MFMA_STRIP_ROWS): an image of h rows enters h rows.  At the bound the matrix kernel is
    planned, one row beyond it the search falls to the stencil kernel."""
    import json
    import subprocess
    import sys

    env = dict(os.environ, WS_MARCH_MFMA="1", WS_MFMA_STRIP_ROWS="1000000")
    out = subprocess.run([sys.executable, "-c", _PLAN_CHILD % ROOT, json.dumps([N, N + 1])], check=True, env=env,
                         capture_output=True, text=True, timeout=120).stdout
    at, beyond = json.loads(out.strip().splitlines()[-1])
    assert at["kernel_kind"] == 1 and at["strips"] == 1 and at["strip_rows"] + WH - 1 == N, at
    assert beyond["kernel_kind"] != 1 and beyond["marching"] == 1, beyond
