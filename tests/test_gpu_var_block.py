"""varBlock (BlockSearch.cpp:125-145, right view), whole maps and the max block size, against the fast exact CPU
reference (oracle.fast_right with var_block, oracle/ws_fast.c, pinned to the line-cited oracle and the NumPy brute
force by tests/test_fast_reference.py).

ws_varblock_kernel runs one wave per pixel: lane l tries min_d + l, min_d + l + 64, ..., keeps a strict < inside the
lane and takes the (cost, d) minimum across lanes.  Here:
  * full-size and real scenes: the config-2 pair with painted flat and quantised patches (wider than 64 px, on every
    border), Teddy and Art at blocks 5 and 7, the reference's pipeline call, a 9 x 9 SAD search in several d-group
    passes;
  * the lane and range seams: D - min_d at 1, 63, 64, 65, 127, 128, 129, 257, a right image narrower than the left;
  * ties inside grown windows (periodic textures, constant images: the smallest d wins, within a lane and across
    lanes) and the growth extremes (thres +inf, 0, -1, -inf, windows past 63);
  * giant windows, whose one row's SSD passes 2^32 or whose block size passes 32767;
  * the entry points: device tensors with padded strides on a torch stream, host calls with padded strides and both
    output types, unequal sizes, the left-right check, a batch, the unrectified search (tests/test_gpu_rectify.py).
"""
import ctypes
import os

import numpy as np
import pytest

from lr_ref import lr_check
from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s)"
                             % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _check(wslib, ctx, oracle, left, right, bs, mind, maxd, smooth=1.0, cost="ssd", thres=19.0, what=""):
    """The device's map and max block against the fast reference; returns the reference's max block."""
    p = wslib.make_params(wslib.VIEW_RIGHT, bs, mind, maxd, smooth, cost, var_block=True, thres=thres)
    got = ctx.search(p, left, right)
    got_mb = ctx.last_max_block(bs)
    want, want_mb = oracle.fast_right(left, right, bs, mind, maxd, smooth=smooth, var_block=True, thres=thres,
                                      cost=cost, return_max_block=True)
    _assert_same(got, want, what)
    assert got_mb == want_mb, (what, got_mb, want_mb)
    return want_mb


def _painted(w, h, maxd, seed, patches, right_width=None):
    """make_pair with flat and quantised (two-level checker) patches painted into L and, along the ground truth, into R:
    there the texture test fails and the windows grow.  patches: (y0, x0, rows, cols, kind)."""
    left, right, gt = make_pair(w, h, maxd, seed, right_width=right_width)
    rw = right.shape[1]
    rng = np.random.default_rng(seed)
    for (y0, x0, ph, pw, kind) in patches:
        ys, xs = np.mgrid[y0:y0 + ph, x0:x0 + pw]
        if kind == "flat":
            val = np.broadcast_to(rng.integers(1, 256, 3, dtype=np.uint8), (ph, pw, 3))
        else:
            a, b = rng.integers(1, 256, (2, 3), dtype=np.uint8)
            val = np.where(((ys // 3 + xs // 5) % 2 == 0)[..., None], a, b).astype(np.uint8)
        left[ys, xs] = val
        tx = xs - gt[ys, xs]
        ok = (tx >= 0) & (tx < rw)
        right[ys[ok], tx[ok]] = val[ok]
    return left, right


def _config2_painted():
    w, h = 1500, 1000
    patches = [(100, 300, 90, 120, "flat"), (400, 700, 70, 200, "quant"), (0, 500, 40, 80, "flat"),
               (h - 50, 900, 50, 90, "quant"), (300, 0, 100, 70, "flat"), (600, w - 80, 120, 80, "flat"),
               (800, 200, 30, 30, "quant"), (0, 0, 35, 35, "flat"), (h - 40, w - 110, 40, 110, "flat")]
    return _painted(w, h, 256, 2, patches)


def _golden_pair(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["left"], z["right"], int(z["ndisp"])


# ---- 1. full size and real scenes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [1.0, 0.9])
def test_config2_with_painted_patches(wslib, gpu_ctx, oracle, smooth):
    """1500 x 1000, 7 x 7 SSD, D = 256: windows grow past 63 in the flat patches (wider than a wave) and along every
    border, so most grown pixels walk four disparities per lane."""
    left, right = _config2_painted()
    mb = _check(wslib, gpu_ctx, oracle, left, right, 7, 0, 256, smooth, "ssd", 19.0, ("config2", smooth))
    assert mb > 63, mb


@pytest.mark.parametrize("bs", [5, 7])
@pytest.mark.parametrize("name", ["teddyH_pair", "artL_pair"])
def test_real_scenes(wslib, gpu_ctx, oracle, name, bs):
    left, right, ndisp = _golden_pair(name)
    mb = _check(wslib, gpu_ctx, oracle, left, right, bs, 0, ndisp, 1.0, "ssd", 19.0, (name, bs))
    assert mb > bs, mb


def test_reference_pipeline_call_on_teddy(wslib, gpu_ctx, oracle):
    """computeDisparityMapRight(17, 0, 200, 0.9, true, 19) through the reference's Python surface."""
    left, right, _ = _golden_pair("teddyH_pair")
    got = wslib.BlockSearch(left, right, 17, 0, 200, context=gpu_ctx).computeDisparityMapRight(0.9, True, 19.0)
    want, want_mb = oracle.fast_right(left, right, 17, 0, 200, smooth=0.9, var_block=True, thres=19.0,
                                      return_max_block=True)
    _assert_same(got, want, "pipeline call")
    assert gpu_ctx.last_max_block(17) == want_mb


def test_sad_9x9_in_several_d_group_passes(wslib, gpu_ctx, oracle):
    """The ordinary search under the grown pixels runs in at least two d-group passes (D from ws_plan)."""
    w, h = 900, 240
    for maxd in (256, 384, 512, 640, 768):
        if wslib.plan(wslib.make_params(wslib.VIEW_RIGHT, 9, 0, maxd, 1.0, "sad"), (h, w), (h, w))["passes"] >= 2:
            break
    else:
        raise AssertionError("no D up to 768 gives two d-group passes at %d x %d" % (w, h))
    left, right = _painted(w, h, maxd, 9, [(20, 600, 80, 150, "flat"), (150, 100, 90, 90, "quant"), (0, 820, 60, 80, "flat")])
    _check(wslib, gpu_ctx, oracle, left, right, 9, 0, maxd, 1.0, "sad", 19.0, ("sad9", maxd))


# ---- 2. lane and range seams ---------------------------------------------------------------------------------------
def _seam_pair(seed, w=420, h=40, right_width=None):
    return _painted(w, h, 64, seed, [(4, 30, 30, 90, "flat"), (10, 200, 24, 70, "quant"), (0, w - 60, 18, 60, "flat")],
                    right_width=right_width)


@pytest.mark.parametrize("mind", [0, 5])
@pytest.mark.parametrize("span", [1, 63, 64, 65, 127, 128, 129, 257])
def test_lane_and_range_seams(wslib, gpu_ctx, oracle, span, mind):
    left, right = _seam_pair(span + mind)
    _check(wslib, gpu_ctx, oracle, left, right, 5, mind, mind + span, 1.0, "ssd", 19.0, (span, mind))


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_right_image_narrower_than_the_left(wslib, gpu_ctx, oracle, cost):
    """d_end = min(max_d - 1, w1 - right - x - 1): with w2 < w1 and D past the width the last columns clip it."""
    left, right = _seam_pair(3, w=300, right_width=260)
    for mind, maxd in ((0, 320), (3, 131)):
        _check(wslib, gpu_ctx, oracle, left, right, 5, mind, maxd, 1.0, cost, 19.0, (cost, mind, maxd))


# ---- 3. ties inside grown windows, growth extremes -----------------------------------------------------------------
def _periodic(w, h, period, seed):
    """A low-contrast texture of horizontal period `period` (the windows grow) in both images: the costs at d and at
    d + k period are equal wherever both are candidates."""
    rng = np.random.default_rng(seed)
    tile = (rng.integers(0, 2, size=(h, period, 3)) + 100).astype(np.uint8)
    img = tile[:, np.arange(w + 8 * period) % period]
    return np.ascontiguousarray(img[:, :w + 8 * period]), np.ascontiguousarray(img[:, :w])


@pytest.mark.parametrize("period", [8, 32, 64])
def test_ties_inside_grown_windows_take_the_smallest_d(wslib, gpu_ctx, oracle, period):
    """min_d 1: the zero-cost candidates are period, 2 period, ...; for period 64 they all sit in lane 63 (a tie
    within one lane), for 8 and 32 in several lanes (ties across lanes).  The smallest d wins."""
    left, right = _periodic(200, 36, period, period)
    for thres, maxd in ((19.0, 200), (40.0, 193)):
        want = oracle.fast_right(left, right, 5, 1, maxd, var_block=True, thres=thres)
        grown = (want != 0)
        assert (want[grown] == period).mean() > 0.5, (period, thres)
        _check(wslib, gpu_ctx, oracle, left, right, 5, 1, maxd, 1.0, "ssd", thres, (period, thres))


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_constant_images_every_candidate_ties(wslib, gpu_ctx, oracle, cost):
    left = np.full((30, 260, 3), 77, np.uint8)
    right = np.full((30, 200, 3), 77, np.uint8)
    for mind, maxd in ((0, 150), (2, 131), (5, 70)):
        mb = _check(wslib, gpu_ctx, oracle, left, right, 3, mind, maxd, 1.0, cost, 19.0, (cost, mind, maxd))
        assert mb > 63, mb


def test_growth_extremes(wslib, gpu_ctx, oracle):
    """thres +inf: every window grows until it stops changing (blocks far past 63); thres 0, -1, -inf: nothing grows,
    the map is the one without varBlock and the max block is the block size."""
    left, right, _ = make_pair(120, 44, 40, seed=21)
    for smooth in (1.0, 0.9):
        mb = _check(wslib, gpu_ctx, oracle, left, right, 5, 0, 40, smooth, "ssd", np.inf, ("inf", smooth))
        assert mb > 63, mb
        plain = oracle.fast_right(left, right, 5, 0, 40, smooth=smooth)
        for thres in (0.0, -1.0, -np.inf):
            assert _check(wslib, gpu_ctx, oracle, left, right, 5, 0, 40, smooth, "sad", thres, (thres, smooth)) == 5
            p = wslib.make_params(wslib.VIEW_RIGHT, 5, 0, 40, smooth, "ssd", var_block=True, thres=thres)
            _assert_same(gpu_ctx.search(p, left, right), plain, ("off", thres, smooth))
            assert gpu_ctx.last_max_block(5) == 5


# ---- 4. giant windows (the issue's scenarios A and B) --------------------------------------------------------------
def _scenario_a():
    """Pixel (1, 22100) grows to block 44101: one row of its window costs more than 2^32 at d = 1..3 (SSD)."""
    right = np.zeros((3, 22200, 3), np.uint8)
    right[1, 22100] = 1
    right[:, 50] = 255
    left = np.full((3, 22210, 3), 255, np.uint8)
    left[:, 50] = 0
    left[:, 1000:1131] = 0
    return left, right


def _scenario_b_wide():
    """Pixel (1, 16450) grows to block 32781: a block size past 16 bits, smoothFactor 0.9 rebuilds its window."""
    right = np.zeros((3, 16500, 3), np.uint8)
    right[1, 16450] = 100
    right[:, 60] = 255
    left = np.zeros((3, 16520, 3), np.uint8)
    left[:, 61] = 255
    return left, right


def _scenario_b_tall():
    right = np.zeros((16500, 3, 3), np.uint8)
    right[16450, 1] = 100
    right[60, :] = 255
    left = np.zeros((16500, 12, 3), np.uint8)
    left[60, 1:3] = 255
    return left, right


@pytest.mark.parametrize("smooth", [1.0, 0.9])
def test_giant_window_row_sum_past_32_bits(wslib, gpu_ctx, oracle, smooth):
    left, right = _scenario_a()
    mb = _check(wslib, gpu_ctx, oracle, left, right, 5, 0, 4, smooth, "ssd", 10.0, ("A", smooth))
    assert mb == 44101
    if smooth == 1.0:    # (at 0.9, d = 0 takes the factor from its black neighbours: 0 under either arithmetic)
        assert oracle.fast_right(left, right, 5, 0, 4, var_block=True, thres=10.0)[1, 22100] == 1


@pytest.mark.parametrize("scene", ["wide", "tall"])
def test_giant_window_block_size_past_16_bits(wslib, gpu_ctx, oracle, scene):
    left, right = _scenario_b_wide() if scene == "wide" else _scenario_b_tall()
    mb = _check(wslib, gpu_ctx, oracle, left, right, 5, 0, 8, 0.9, "ssd", 200.0, ("B", scene))
    assert mb == 32781
    yx = (1, 16450) if scene == "wide" else (16450, 1)
    assert oracle.fast_right(left, right, 5, 0, 8, smooth=0.9, var_block=True, thres=200.0)[yx] == 1


# ---- 5. entry points -----------------------------------------------------------------------------------------------
def _entry_pair(seed, w=260, h=70, right_width=None, right_height=None):
    left, right, gt = make_pair(w, h, 96, seed, right_width=right_width, right_height=right_height)
    left[10:50, 40:140] = 90                                     # flat in both (grown windows, d past 64)
    right[10:min(50, right.shape[0]), 0:100] = 90
    return left, right


def test_device_tensors_with_padded_strides_on_a_stream(wslib, gpu_ctx, oracle):
    import torch
    left, right = _entry_pair(31)
    h, w = right.shape[:2]
    tl = torch.zeros((left.shape[0], left.shape[1] + 13, 3), dtype=torch.uint8, device="cuda")
    tr = torch.zeros((h, w + 7, 3), dtype=torch.uint8, device="cuda")
    tl[:, :left.shape[1]] = torch.from_numpy(left).cuda()
    tr[:, :w] = torch.from_numpy(right).cuda()
    to = torch.full((h, w + 21), -7.0, dtype=torch.float32, device="cuda")
    vl, vr, vo = tl[:, :left.shape[1]], tr[:, :w], to[:, :w]
    stream = torch.cuda.Stream()
    for smooth, maxd in ((1.0, 130), (0.9, 96)):
        p = wslib.make_params(wslib.VIEW_RIGHT, 7, 0, maxd, smooth, "ssd", var_block=True, thres=19.0)
        with torch.cuda.stream(stream):
            gpu_ctx.search_device(p, vl, vr, vo, stream.cuda_stream)
        stream.synchronize()
        want, want_mb = oracle.fast_right(left, right, 7, 0, maxd, smooth=smooth, var_block=True, thres=19.0,
                                          return_max_block=True)
        _assert_same(vo.cpu().numpy().astype(np.float64), want, ("device", smooth))
        assert (to[:, w:].cpu().numpy() == -7.0).all()            # the padding stays untouched
        assert gpu_ctx.last_max_block(7) == want_mb and want_mb > 7


def test_host_calls_with_padded_strides_and_both_output_types(wslib, gpu_ctx, oracle):
    lib = wslib.load_library()
    left, right = _entry_pair(32)
    h, w = right.shape[:2]
    bl = np.zeros((left.shape[0], left.shape[1] + 5, 3), np.uint8)
    br = np.zeros((h, w + 9, 3), np.uint8)
    bl[:, :left.shape[1]], br[:, :w] = left, right
    Li = wslib._Image(bl.ctypes.data, left.shape[1], left.shape[0], bl.strides[0])
    Ri = wslib._Image(br.ctypes.data, w, h, br.strides[0])
    want, want_mb = oracle.fast_right(left, right, 5, 2, 150, var_block=True, thres=25.0, return_max_block=True)
    p = wslib.make_params(wslib.VIEW_RIGHT, 5, 2, 150, 1.0, "ssd", var_block=True, thres=25.0)
    for dtype, code in ((np.float32, wslib.OUT_F32), (np.float64, wslib.OUT_F64)):
        out = np.full((h, w + 11), -3.0, dtype=dtype)
        rc = lib.ws_search_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), out.ctypes.data,
                                w + 11, code)
        assert rc == 0, lib.ws_last_error(gpu_ctx._h)
        _assert_same(out[:, :w].astype(np.float64), want, dtype)
        assert (out[:, w:] == -3.0).all()
        assert gpu_ctx.last_max_block(5) == want_mb


@pytest.mark.parametrize("shape", [(300, 70, 260, 70), (240, 70, 280, 70), (260, 74, 260, 66), (300, 72, 250, 64)])
def test_unequal_sizes(wslib, gpu_ctx, oracle, shape):
    """Wider left, wider right, a taller left image, both at once (a taller right image is refused with varBlock)."""
    w1, h1, w2, h2 = shape
    left, right = _entry_pair(33 + w2, w1, h1, right_width=w2, right_height=h2)
    for smooth in (1.0, 0.9):
        _check(wslib, gpu_ctx, oracle, left, right, 7, 0, 140, smooth, "ssd", 19.0, (shape, smooth))


def test_search_lr_host_with_var_block(wslib, gpu_ctx, oracle):
    left, right = _entry_pair(34)
    dl = oracle.fast_left(left, right, 7, 0, 128).astype(np.float32)
    dr = oracle.fast_right(left, right, 7, 0, 128, var_block=True, thres=19.0).astype(np.float32)
    p = wslib.make_params(wslib.VIEW_RIGHT, 7, 0, 128, 1.0, "ssd", var_block=True, thres=19.0)
    for md, fill in ((1.0, False), (0.0, True)):
        want_l, want_r, want_c = lr_check(dl, dr, md, fill)
        got_l, got_r = gpu_ctx.search_lr(p, left, right, md, fill, dtype=np.float32)
        assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32)), (md, fill)
        assert np.array_equal(got_r.view(np.uint32), want_r.view(np.uint32)), (md, fill)
        assert gpu_ctx.last_lr_counts() == want_c


def test_batch_of_var_block_jobs_goes_whole_pair(wslib, gpu_ctx, oracle):
    pairs = [_entry_pair(40 + k, 240 + 16 * k, 300 + 20 * k) for k in range(4)]
    plist = [wslib.make_params(wslib.VIEW_RIGHT, 5 + 2 * (k % 2), 0, 100 + 10 * k, 1.0, "ssd", var_block=True,
                               thres=19.0) for k in range(4)]
    with wslib.BatchSearch([0, 0]) as b:
        items, banded = b.plan(plist, pairs, bands=True, min_rows=64)
        assert not banded and sorted(it[0] for it in items) == list(range(len(pairs)))
        got = b.search(plist, pairs, dtype=np.float64, bands=True, min_rows=64)
    for k, ((left, right), g) in enumerate(zip(pairs, got)):
        want = oracle.fast_right(left, right, 5 + 2 * (k % 2), 0, 100 + 10 * k, var_block=True, thres=19.0)
        _assert_same(g, want, k)
