"""The matrix-core SSD kernel (csrc/ws_march_mfma.h: `ws_march_kernel<ssd,7x7,mfma>`), whole maps against the fast exact
CPU reference (oracle.fast_left), np.array_equal.  Every case asserts that the matrix kernel ran, so none can pass on the
stencil kernel:

  * config 2's shape; max_disparity 33 / 100 / 255 / 256 (partial first and last tiles of target centres, the poisoned
    triangles of candidates outside the range) and the narrowest search the selection rule gives the kernel;
  * widths and heights, found by scanning ws_plan, that put the image edge 1 and tile - 1 columns / 1 and strip - 1 rows
    past a seam;
  * inputs where only the tie tags decide (constant, constant_apart, extremes, saturated, periodic) and the maximum-cost
    pairs (255 against 0: -128 / 127 and the complement at the int8 limits);
  * device images at every base address & 15 and row strides of every phase, unequal left / right sizes, black pixels;
  * the same map from search_device, the banded host path and, in a child process, WS_MARCH_MFMA=0 (the stencil kernel).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 7
MFMA = "ws_march_kernel<ssd,7x7,mfma>"


def _params(wslib, maxd):
    return wslib.make_params(wslib.VIEW_LEFT, BS, 0, maxd, 1.0, "ssd")


def _plan(wslib, maxd, w, h):
    return wslib.plan(_params(wslib, maxd), (h, w, 3), (h, w, 3))


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s)"
                             % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _run(wslib, ctx, oracle, left, right, maxd, what):
    got = ctx.search(_params(wslib, maxd), left, right)
    info = ctx.last_launch()
    assert "mfma" in info["kernel"] and info["kernel"] == MFMA, (what, info)
    _assert_same(got, oracle.fast_left(left, right, BS, 0, maxd, cost="ssd"), what)
    return got


def test_config2_whole_map(wslib, gpu_ctx, oracle):
    left, right, _ = make_pair(1500, 1000, 256, 2)
    p = _plan(wslib, 256, 1500, 1000)
    assert p["kernel_kind"] == 1 and p["threads"] == 512 and p["tile_cols"] == 128 and p["passes"] == 1, p
    _run(wslib, gpu_ctx, oracle, left, right, 256, "config2")


@pytest.mark.parametrize("maxd", [33, 100, 255, 256])
def test_disparity_ranges(wslib, gpu_ctx, oracle, maxd):
    w, h = 700, 300
    left, right, _ = make_pair(w, h, maxd, 40 + maxd)
    left[h // 2, w // 3:w // 3 + 5] = 0                  # a few black pixels on each side
    right[h // 3, w // 2:w // 2 + 5] = 0
    _run(wslib, gpu_ctx, oracle, left, right, maxd, ("maxd", maxd))


def test_narrowest_selected_search(wslib, gpu_ctx, oracle):
    """The narrowest search the selection rule still gives the kernel: of all the searches it sees, the one with the
    most target centres of its first tiles outside the image.  (The clamp of the candidate range by the width,
    d_hi = width - 7, cannot be reached: the rule needs 390 columns, max_disparity + the window is at most 262.)"""
    found = None
    for w in range(200, 700):
        for h in (200, 260, 400):
            if _plan(wslib, 256, w, h)["kernel_kind"] == 1:
                found = (w, h)
                break
        if found:
            break
    assert found, "no search narrower than 700 columns selects the matrix kernel"
    w, h = found
    left, right, _ = make_pair(w, h, 256, 77)
    _run(wslib, gpu_ctx, oracle, left, right, 256, ("narrowest", w, h))


@pytest.mark.parametrize("seam", ["strip_1", "strip_m1", "tile_1", "tile_m1"])
def test_seams(wslib, gpu_ctx, oracle, seam):
    maxd = 200
    if seam.startswith("strip"):
        scan = [(w, h) for w in (600, 900) for h in range(200, 900)]
    else:
        scan = [(w, 300) for w in range(400, 1700)]
    found = None
    for w, h in scan:
        p = _plan(wslib, maxd, w, h)
        if p["kernel_kind"] != 1:
            continue
        if seam.startswith("strip"):
            if p["strips"] < 2 or p["strip_rows"] < 3:
                continue
            last = (p["interior_y1"] - p["interior_y0"]) - (p["strips"] - 1) * p["strip_rows"]
            want = 1 if seam == "strip_1" else p["strip_rows"] - 1
        else:
            if p["tiles"] < 2:
                continue
            last = (p["interior_x1"] - p["interior_x0"]) - (p["tiles"] - 1) * p["tile_cols"]
            want = 1 if seam == "tile_1" else p["tile_cols"] - 1
        if last == want:
            found = (w, h, p)
            break
    if not found:
        pytest.fail("the planner gives the matrix kernel no shape with seam %s" % seam)
    w, h, p = found
    left, right, _ = make_pair(w, h, maxd, 900 + len(seam))
    left[h // 2, w // 3:w // 3 + 5] = 0
    right[h // 3, w // 2:w // 2 + 5] = 0
    _run(wslib, gpu_ctx, oracle, left, right, maxd, (seam, w, h, p))


def _tie_pair(kind, w, h, seed):
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


@pytest.mark.parametrize("kind", ["constant", "constant_apart", "extremes", "saturated", "periodic"])
def test_ties_whole_map(wslib, gpu_ctx, oracle, kind):
    w, h, maxd = 600, 230, 256
    left, right = _tie_pair(kind, w, h, seed=7 * 7 + maxd)
    _run(wslib, gpu_ctx, oracle, left, right, maxd, kind)


P_HI = np.array([255, 0, 255], np.uint8)     # neither pixel is black, every channel differs by 255
P_LO = np.array([0, 255, 0], np.uint8)


def _extreme_pair(w, h, kind, rng):
    left = np.broadcast_to(P_HI, (h, w, 3)).copy()
    right = np.broadcast_to(P_LO, (h, w, 3)).copy()
    if kind == "one_below":                  # a few pixels one unit closer: their windows cost the maximum - 509 and win
        for _ in range(3):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            right[y, x, 1] = 254
            left[int(rng.integers(h)), int(rng.integers(w)), 0] = 254
    elif kind == "columns":                  # alternating columns: every other candidate costs 0, the rest the maximum
        left[:, 1::2] = P_LO
        right[:, 1::2] = P_HI
    return left, right


@pytest.mark.parametrize("kind", ["all_max", "one_below", "columns"])
def test_maximum_cost_windows(wslib, gpu_ctx, oracle, kind):
    rng = np.random.default_rng(5)
    left, right = _extreme_pair(640, 210, kind, rng)
    _run(wslib, gpu_ctx, oracle, left, right, 256, kind)


def test_device_images_at_every_alignment(wslib, gpu_ctx, oracle):
    """search_device on views into larger byte buffers: base address & 15 = 0 .. 15 for each image in turn, row strides
    that walk through every phase modulo 16 (and so every byte phase of a column modulo 4), unequal sizes, black pixels."""
    import torch
    w1, h1, w2, h2, maxd = 530, 211, 547, 226, 140
    left, right, _ = make_pair(w1, h1, maxd, 31, right_width=w2, right_height=h2)
    left[:, :30] = 0
    left[:12] = 0
    right[:, w2 - 40:] = 0
    right[h2 - 20:] = 0
    left[100, 200:260] = 0
    p = _params(wslib, maxd)
    assert wslib.plan(p, left.shape, right.shape)["kernel_kind"] == 1
    want = oracle.fast_left(left, right, BS, 0, maxd, cost="ssd")

    def view(img, off, stride):
        h, w = img.shape[:2]
        buf = torch.zeros(off + stride * h + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        t = torch.as_strided(buf, (h, w, 3), (stride, 3, 1), off)
        t.copy_(torch.from_numpy(img))
        return buf, t

    out = torch.empty((h1, w1), dtype=torch.float32, device="cuda")
    for k in range(16):
        # strides 3 w + 1 + k: odd and even, every residue modulo 16 over the sweep
        bl, tl = view(left, k, 3 * w1 + 1 + k)
        br, tr = view(right, (5 * k + 3) % 16, 3 * w2 + 16 - k)
        out.fill_(-7.0)
        gpu_ctx.search_device(p, tl, tr, out, None)
        torch.cuda.synchronize()
        assert gpu_ctx.last_launch()["kernel"] == MFMA, gpu_ctx.last_launch()
        _assert_same(out.cpu().numpy().astype(np.float64), want, ("alignment", k))


def test_unequal_pair_with_black_margins(wslib, gpu_ctx, oracle):
    w1, h1, w2, h2, maxd = 1481, 1038, 1495, 1052, 140
    left, right, _ = make_pair(w1, h1, maxd, 31, right_width=w2, right_height=h2)
    left[:, :30] = 0
    left[:12] = 0
    right[:, w2 - 40:] = 0
    right[h2 - 20:] = 0
    _run(wslib, gpu_ctx, oracle, left, right, maxd, "unequal")


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import stereo_reconstruction_amd as ws
from stereo_reconstruction_amd.synthetic import make_pair
left, right, _ = make_pair(900, 800, 256, 11)
p = ws.make_params(ws.VIEW_LEFT, 7, 0, 256, 1.0, "ssd")
assert ws.plan(p, left.shape, right.shape)["kernel_kind"] == 0
with ws.WindowSearch(0) as ctx:
    got = ctx.search(p, left, right)
    name = ctx.last_launch()["kernel"]
assert "march" in name and "mfma" not in name, name
np.save(sys.argv[1], got)
"""


def test_same_map_from_every_path(wslib, gpu_ctx, oracle, tmp_path):
    import torch
    w, h, maxd = 900, 800, 256   # (three bands: the first and the last are half bands of 200 rows)
    left, right, _ = make_pair(w, h, maxd, 11)
    p = _params(wslib, maxd)
    gpu_ctx.set_host_bands(0)
    try:
        plain = _run(wslib, gpu_ctx, oracle, left, right, maxd, "plain host call")
        for nb in (2, 3):
            gpu_ctx.set_host_bands(nb)
            got = gpu_ctx.search(p, left, right)
            assert gpu_ctx.last_launch()["kernel"] == MFMA, gpu_ctx.last_launch()
            _assert_same(got, plain, ("bands", nb))
    finally:
        gpu_ctx.set_host_bands(-1)
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    gpu_ctx.search_device(p, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), out, None)
    torch.cuda.synchronize()
    assert gpu_ctx.last_launch()["kernel"] == MFMA
    _assert_same(out.cpu().numpy().astype(np.float64), plain, "search_device")
    # the stencil kernel, in a process that never plans the matrix kernel
    path = str(tmp_path / "stencil.npy")
    env = dict(os.environ, WS_MARCH_MFMA="0")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, path], check=True, env=env, timeout=600)
    _assert_same(np.load(path), plain, "WS_MARCH_MFMA=0")
