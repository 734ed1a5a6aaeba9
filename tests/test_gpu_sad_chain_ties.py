"""The SSD marching kernel's v_sad_u32 chain (ws_march_kernel.h, march_sadp) where only the tie tags decide: its tags
live in the bias operand and are decoded per column by the flush, so inputs whose candidates tie -- constant images,
periodic textures, 0 / 255 extremes -- are compared whole against the fast exact CPU reference (oracle.fast_left /
fast_right), left view 7 x 7 and 9 x 9, right view 6 x 6 and 8 x 8 (block sizes 7 and 9), one d-group pass and
several (D = 1024: the key plane between passes).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pair(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "constant":                       # every candidate of a pixel costs 0
        return np.full((h, w, 3), 77, np.uint8), np.full((h, w, 3), 77, np.uint8)
    if kind == "constant_apart":                 # every candidate costs the same nonzero amount
        return np.full((h, w, 3), 200, np.uint8), np.full((h, w, 3), 13, np.uint8)
    if kind == "extremes":                       # 255 against 0: the largest cost a window can have, everywhere
        return np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    if kind == "saturated":                      # 0 / 255 per pixel: black pixels and maximum-cost windows
        left = np.repeat(rng.integers(0, 2, (h, w, 1)) * 255, 3, axis=2).astype(np.uint8)
        right = np.repeat(rng.integers(0, 2, (h, w, 1)) * 255, 3, axis=2).astype(np.uint8)
        return left, right
    if kind == "periodic":                       # ties between candidates a period apart
        x = np.arange(w)
        row = np.stack([(x % 5) * 50 + 10, (x % 3) * 80 + 20, (x % 15) * 16 + 5], axis=-1).astype(np.uint8)
        left = np.broadcast_to(row, (h, w, 3)).copy()
        return left, np.roll(left, 2, axis=1).copy()
    raise ValueError(kind)


@pytest.mark.parametrize("maxd", [64, 1024])
@pytest.mark.parametrize("kind", ["constant", "constant_apart", "extremes", "saturated", "periodic"])
@pytest.mark.parametrize("bs", [7, 9])
@pytest.mark.parametrize("view", ["left", "right"])
def test_ssd_ties_whole_map(wslib, gpu_ctx, oracle, view, bs, kind, maxd):
    w, h = (1100, 24) if maxd > 512 else (300, 30)
    left, right = _pair(kind, w, h, seed=bs * 7 + maxd)
    win = bs if view == "left" else bs - 1       # the right view's window is (bs - 1) x (bs - 1)
    p = wslib.make_params(wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT, bs, 0, maxd, 1.0, "ssd")
    got = gpu_ctx.search(p, left, right)
    kernel = gpu_ctx.last_launch()["kernel"]
    assert "ssd,%dx%d" % (win, win) in kernel, kernel
    want = (oracle.fast_left if view == "left" else oracle.fast_right)(left, right, bs, 0, maxd, cost="ssd")
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%d pixels differ, first %s (got %s, want %s)"
                             % (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
