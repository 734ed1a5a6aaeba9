"""Inputs of the census-cost tests, shared by the reference tests (which show on the reference alone that they do what
they claim) and the device tests.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from test_subpixel_reference import shifted_pair


def grey3(a):
    """An H x W array of grey levels as a BGR image (B = G = R)."""
    return np.repeat(np.asarray(a, dtype=np.uint8)[:, :, None], 3, axis=2)


def random_pair(w, h, seed, w2=None, h2=None):
    """Independent random colours in 1..255 (nothing black), the right image of its own size."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 256, size=(h, w, 3)).astype(np.uint8)
    R = rng.integers(1, 256, size=(h2 or h, w2 or w, 3)).astype(np.uint8)
    return L, R


def textured_pair(w, h, t, seed, w2=None, h2=None, black=False):
    """R(y, x) = L(y, x + t) with a little noise; optionally a right image of another size, black pixels and a black row."""
    L, R = shifted_pair(max(w, (w2 or w)), h if h2 is None else max(h, h2), t, seed, right_width=w2 or w)
    L, R = L[:h, :w].copy(), R[:(h2 or h)].copy()
    if black:
        for img in (L, R):
            hh, ww = img.shape[:2]
            img[hh // 3: hh // 3 + 3, ww // 4: ww // 4 + 9] = 0
            img[(2 * hh) // 3] = 0
    return L, R


def inverted_pair(seed=5):
    """A random grey L in 1..255, 80 x 48, and R(x) = 255 - L(x + 4) (columns wrap): inverting the grey order flips
    nearly every descriptor bit, so the window costs come close to their bound bits * block_size^2."""
    rng = np.random.default_rng(seed)
    l = rng.integers(1, 256, size=(48, 80))
    r = 255 - np.roll(l, -4, axis=1)
    return grey3(l), grey3(r)


def periodic_pair(w=61, h=23, period=4):
    """An image periodic in x: every disparity that is a multiple of the period ties."""
    row = (np.arange(w) % period) * 50 + 30
    img = grey3(np.broadcast_to(row, (h, w)) + (np.arange(h) % 3)[:, None] * 7)
    return img, img.copy()


def lut_pair(w, h, t, seed):
    """A grey pair with levels in 1..120 and the lookup table v -> 2 v + 10 (strictly increasing on them, into 12..250)."""
    L, R = shifted_pair(w, h, t, seed)
    l, r = (L[:, :, 0] % 120 + 1), (R[:, :, 0] % 120 + 1)
    lut = (2 * np.arange(256) + 10).clip(0, 255).astype(np.uint8)
    return grey3(l), grey3(r), lut
