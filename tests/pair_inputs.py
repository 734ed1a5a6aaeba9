"""Inputs of the device tests of the pair call (tests/test_gpu_pair.py), and their references, computed once per case.
TEST INFRASTRUCTURE ONLY.  tests/test_pair_inputs.py shows on the reference alone that they bite: periodic pairs whose
derived map is decided by the tie rule, staircases whose derived winners fall in every 64-lane chunk of a curve, and
every class of derived pixel.
"""
import functools
import os
import re
import zlib

import numpy as np

from conftest import ROOT
from pair_ref import derived_np, other_shape
from sgm_inputs import nd_of, staircase_pair, staircase_width
from unique_ref import sums, volume


def kernel_constant(name):
    """A constexpr int of csrc/ws_sgm.h (kPairSpan, kPairSwitchWidth), resolved through one level of naming."""
    text = open(os.path.join(ROOT, "stereo_reconstruction_amd", "csrc", "ws_sgm.h")).read()
    m = re.search(r"constexpr int %s = (\w+);" % name, text)
    return int(m.group(1)) if m.group(1).isdigit() else kernel_constant(m.group(1))


def periodic_pair(w, h, period, seed):
    """A random cell of `period` columns tiled along the row, L(x) = R(x - 2): every disparity 2 + k period matches
    exactly, so a derived pixel's candidates tie and the tie rule alone decides."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(1, 256, size=(h, period, 3)).astype(np.uint8)
    T = np.tile(cell, (1, (w + 2) // period + 2, 1))
    return np.ascontiguousarray(T[:, :w]), np.ascontiguousarray(T[:, 2:w + 2])


# name: (w, h, period, max_disparity): 3 x 3 SAD, min_disparity 0, sgm None and (4, 0, 0)
PERIODIC = {"150x9": (150, 9, 7, 130), "97x8": (97, 8, 5, 200)}


@functools.lru_cache(maxsize=None)
def periodic_case(name):
    w, h, period, maxd = PERIODIC[name]
    return periodic_pair(w, h, period, zlib.crc32(name.encode()) & 0xffff) + (maxd,)


# name: (view, cost, block_size, min_d, nd, h, paths, p1, p2): both bases at nd = 129, 257, 1025 and 2048.  The left
# ones are sgm_inputs.STAIRCASES' own; the P2 of the wide ones keeps S in 32 bits so that the references stay quick.
STAIRCASES = {
    "129-left": ("left", "sad", 3, 0, 129, 4, 8, 20, 400),
    "129-right": ("right", "sad", 3, 0, 129, 4, 8, 20, 400),
    "257-left": ("left", "ssd", 1, 0, 257, 6, 8, 50, 3000),
    "257-right": ("right", "ssd", 3, 1, 257, 4, 4, 50, 3000),
    "1025-left": ("left", "ssd", 1, 0, 1025, 3, 4, 50, 1_100_000_000),
    "1025-right": ("right", "sad", 3, 1, 1025, 3, 8, 20, 600_000_000),
    "2048-left": ("left", "sad", 3, 0, 2048, 3, 4, 20, 1_000_000_000),
    "2048-right": ("right", "ssd", 3, 0, 2048, 3, 4, 300, 1_000_000_000),
}


@functools.lru_cache(maxsize=None)
def staircase_case(name):
    """(L, R, (view, bs, mind, maxd, cost), (paths, p1, p2), nd) of a case of STAIRCASES."""
    view, cost, bs, mind, nd, h, paths, p1, p2 = STAIRCASES[name]
    half = (bs - 1) // 2
    lo = 1 if view == "left" else mind
    top = nd if view == "left" else mind + nd - 1
    maxd = nd if view == "left" else mind + nd
    w = staircase_width(top, half)
    L, R = staircase_pair(w, h, lo, top, zlib.crc32(name.encode()) & 0xffff, view)
    assert nd_of(view, bs, mind, maxd, w) == nd
    return L, R, (view, bs, mind, maxd, cost), (paths, p1, p2), nd


@functools.lru_cache(maxsize=None)
def sums_of(L_bytes, R_bytes, lshape, rshape, view, bs, mind, maxd, cost, sgm):
    L = np.frombuffer(L_bytes, np.uint8).reshape(lshape)
    R = np.frombuffer(R_bytes, np.uint8).reshape(rshape)
    V = volume(L, R, view, bs, mind, maxd, cost)
    return V, sums(V, sgm)


def case_sums(L, R, view, bs, mind, maxd, cost, sgm):
    """(V, S) of the base view, shared (read only) by the tests that need them."""
    return sums_of(L.tobytes(), R.tobytes(), L.shape, R.shape, view, bs, mind, maxd, cost, sgm)


def derived_of(L, R, view, bs, mind, maxd, cost, sgm, tie="rule", winners=False):
    V, S = case_sums(L, R, view, bs, mind, maxd, cost, sgm)
    return derived_np(S, V[1], view, other_shape(L, R, view), tie, winners)


def candidate_counts(S, d0, view, shape):
    """The number of candidates of every derived pixel."""
    from sgm_ref import BIG
    nd, h, w = S.shape
    ho, wo = shape
    rows = min(h, ho)
    n = np.zeros((ho, wo), dtype=np.int64)
    xs = np.arange(w)
    for j in range(nd):
        c = xs - (d0 + j) if view == "left" else xs + (d0 + j)
        ok = (c >= 0) & (c < wo)
        n[:rows, c[ok]] += S[j, :rows][:, ok] < BIG
    return n
