"""The census-transform matching cost on the device: descriptors, whole block-search maps and SGM maps bit for bit
against tests/census_cost_ref.py (every float32 sub-pixel value included, no pixel left out), and every caller of the
search dispatch.

The seams of the kernels (ws_ct.hip) the shapes cross: the transform's tiles of 32 x 8 pixels; the match kernel's tiles of
64 columns (16 per wave) and strips of 32 rows; its chunks of 62 owned candidates (winner-take-all sink: seams at j = 62,
124, ...) and of 64 (SGM's cost sink); the 16-bit / 32-bit cost store.  131 x 37 and 197 x 70 have more than one tile,
strip and wave run in each direction and end inside one; block 63 is larger than the 37-row image and leaves 7 rows of
the 70-row one.
"""
import os
import subprocess

import numpy as np
import pytest

from census_cost_inputs import inverted_pair, lut_pair, periodic_pair, random_pair, textured_pair
from census_cost_ref import slice_volume, transform_np, volume, wta
from conftest import ROOT, load_golden
from lr_ref import lr_check
from sgm_ref import sgm_from_volume

pytestmark = pytest.mark.gpu

COSTS = ["census5x5", "census9x7"]
VIEWS = ["left", "right"]
MATCH_KERNEL = "ws_census_match_kernel"


def _torch():
    import torch
    return torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:5].tolist(), [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:3]]))


def dev_image(torch, a, pad=0):
    """a (H x W x 3 uint8) in a CUDA tensor whose rows are 3 (W + pad) bytes apart."""
    h, w = a.shape[:2]
    t = torch.full((h, w + pad, 3), 77, dtype=torch.uint8, device="cuda")
    t[:, :w] = torch.from_numpy(np.ascontiguousarray(a))
    return t[:, :w]


def params_of(wslib, view, bs, mind, maxd, cost, subpixel=False):
    return wslib.make_params(wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT, bs, mind, maxd, cost=cost, subpixel=subpixel)


class Device:
    """A pair on the device (padded rows) and a padded output, reused over the searches of a case."""

    def __init__(self, wslib, ctx, L, R, view, pad=5):
        torch = _torch()
        self.wslib, self.ctx, self.view, self.pad = wslib, ctx, view, pad
        self.tl, self.tr = dev_image(torch, L, pad), dev_image(torch, R, pad)
        self.h, self.w = (L if view == "left" else R).shape[:2]
        self.out = torch.empty((self.h, self.w + pad), dtype=torch.float32, device="cuda")

    def _result(self):
        torch = _torch()
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        assert np.isnan(o[:, self.w:]).all(), "the padding of the output rows was written"
        return o[:, :self.w]

    def search(self, p, stream=None):
        self.out.fill_(float("nan"))
        _torch().cuda.synchronize()
        self.ctx.search_device(p, self.tl, self.tr, self.out[:, :self.w], stream=stream)
        return self._result()

    def sgm(self, p, paths, p1, p2):
        self.out.fill_(float("nan"))
        _torch().cuda.synchronize()
        self.ctx.search_sgm_device(p, self.tl, self.tr, self.out[:, :self.w], paths, p1, p2)
        return self._result()


# ---- the transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (2, 3), (9, 7), (131, 37), (197, 70)])
def test_transform_host_and_device_equal_the_reference(wslib, gpu_ctx, cost, w, h):
    torch = _torch()
    img, _ = random_pair(w, h, 31 * w + h)
    if w > 8:
        img[h // 2, w // 3: w // 3 + 4] = img[h // 2, w // 3]      # equal neighbours: ties give 0 bits
    want = transform_np(img, cost)
    got = gpu_ctx.census_transform(img, cost)
    assert got.dtype == np.uint64 and got.tobytes() == want.tobytes()
    assert gpu_ctx.census_transform(img, wslib._COST[cost]).tobytes() == want.tobytes()
    t = dev_image(torch, img, pad=3)                               # a stride wider than 3 w
    out = torch.full((h, w + 6), -1, dtype=torch.int64, device="cuda")
    gpu_ctx.census_transform_device(t, cost, out[:, :w])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, w:] == -1).all(), "the padding of the output rows was written"
    assert o[:, :w].astype(np.uint64).tobytes() == want.tobytes()
    with pytest.raises(wslib.WsError) as e:
        gpu_ctx.census_transform(img, wslib.COST_SAD)
    assert e.value.code == -1


# ---- the search ------------------------------------------------------------------------------------------------------
MAXD = [1, 2, 63, 64, 65, 130, 257, 5000]


def check_searches(wslib, ctx, L, R, view, cost, blocks, minds, maxds=MAXD, subs=(False, True)):
    dev = Device(wslib, ctx, L, R, view)
    for bs in blocks:
        for mind in minds:
            big = volume(L, R, view, bs, mind, max(maxds), cost)   # once per (block, minD); smaller ranges are its prefixes
            for maxd in maxds:
                nd = min(maxd, big[0].shape[0]) if view == "left" else min(max(0, maxd - mind), big[0].shape[0])
                V = slice_volume(big, nd)
                for sub in subs:
                    got = dev.search(params_of(wslib, view, bs, mind, maxd, cost, sub))
                    assert_bits(got, wta(V, view, sub), (view, cost, bs, mind, maxd, sub, L.shape, R.shape))


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("w,h", [(131, 37), (197, 70)])
def test_search_every_block_and_range(wslib, gpu_ctx, view, cost, w, h):
    L, R = textured_pair(w, h, 9, w + h, black=True)
    check_searches(wslib, gpu_ctx, L, R, view, cost, (1, 3, 7, 17, 63), (0,))
    if view == "right":
        check_searches(wslib, gpu_ctx, L, R, view, cost, (3, 17), (3,))
    assert gpu_ctx.last_launch()["kernel"] == MATCH_KERNEL


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
def test_search_right_image_of_another_size(wslib, gpu_ctx, view, cost):
    """Narrower and shorter, wider, and (one row) taller and wider than the left image; black pixels and a black row."""
    for k, (w2, h2) in enumerate(((122, 33), (142, 37), (140, 38))):
        L, R = textured_pair(131, 37, 7, 40 + k, w2=w2, h2=h2, black=True)
        assert R.shape[:2] == (h2, w2) and L.shape[:2] == (37, 131)
        check_searches(wslib, gpu_ctx, L, R, view, cost, (3, 7), (0, 3) if view == "right" else (0,), maxds=(2, 64, 5000))


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
def test_search_tiny_images_and_blocks_larger_than_the_image(wslib, gpu_ctx, view, cost):
    for w, h in ((1, 1), (3, 2), (9, 7)):
        L, R = random_pair(w, h, 77 + w)
        check_searches(wslib, gpu_ctx, L, R, view, cost, (1, 3, 17), (0,), maxds=(1, 5, 64))


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
def test_ties(wslib, gpu_ctx, view, cost):
    """A constant image (every cost 0) and an image periodic in x with period 4: the view's tie rule decides, also across
    the chunks of the disparity range."""
    const = np.full((37, 150, 3), 90, np.uint8)
    P, Q = periodic_pair(150, 37)
    for A, B in ((const, const.copy()), (P, Q)):
        check_searches(wslib, gpu_ctx, A, B, view, cost, (1, 5), (0, 3) if view == "right" else (0,), maxds=(16, 64, 140))


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
def test_invariance_under_a_strictly_increasing_map(wslib, gpu_ctx, view, cost):
    L, R, lut = lut_pair(131, 37, 6, 21)
    want = wta(volume(L, R, view, 7, 0, 40, cost), view, True)
    p = params_of(wslib, view, 7, 0, 40, cost, True)
    for A, B in ((L, R), (L, lut[R]), (lut[L], R), (lut[L], lut[R])):
        assert_bits(Device(wslib, gpu_ctx, A, B, view).search(p), want, (view, cost))
    sad = params_of(wslib, view, 7, 0, 40, "sad")
    assert (Device(wslib, gpu_ctx, L, R, view).search(sad) != Device(wslib, gpu_ctx, L, lut[R], view).search(sad)).any()


# ---- semi-global matching --------------------------------------------------------------------------------------------
PENALTIES = [(0, 0), (3, 20), (10, 120)]


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("nd", [1, 64, 65, 200])
def test_sgm(wslib, gpu_ctx, view, cost, nd):
    w, h, bs = nd + 31, 35, 5
    L, R = textured_pair(w, h, max(1, min(nd // 2, 9)), nd, black=True)
    mind = 0 if view == "left" else 2
    maxd = nd if view == "left" else nd + mind
    V = volume(L, R, view, bs, mind, maxd, cost)
    assert V[0].shape[0] == nd
    dev = Device(wslib, gpu_ctx, L, R, view)
    for paths in (4, 8):
        for k, (p1, p2) in enumerate(PENALTIES):
            sub = (k + paths) % 2 == 0
            p = params_of(wslib, view, bs, mind, maxd, cost, sub)
            got = dev.sgm(p, paths, p1, p2)
            assert_bits(got, sgm_from_volume(V, view, paths, p1, p2, sub), (view, cost, nd, paths, p1, p2, sub))
            if p2 == 0:      # the identity: the census block search itself, bit for bit
                assert_bits(got, dev.search(p), ("identity", view, cost, nd, paths, sub))


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("bs", [31, 33])
def test_sgm_inverted_pair_at_the_16_bit_bound(wslib, gpu_ctx, view, bs):
    """9x7 costs fit 16 bits at block size 31 and pass 65535 at 33 (tests/test_census_cost_reference.py shows both, and
    that a 16-bit cut changes the map)."""
    L, R = inverted_pair()
    V = volume(L, R, view, bs, 0, 64, "census9x7")
    # (the right view's clipped window has 2 half columns and rows: 62 * 32 * 32 < 65536 even at block size 33, where the
    # host's bound on a full block already stores 32 bits)
    assert (V[0].max() > 65535) == (bs == 33 and view == "left")
    dev = Device(wslib, gpu_ctx, L, R, view)
    for sub in (False, True):
        p = params_of(wslib, view, bs, 0, 64, "census9x7", sub)
        assert_bits(dev.sgm(p, 8, 3, 20), sgm_from_volume(V, view, 8, 3, 20, sub), (view, bs, sub))
        assert_bits(dev.sgm(p, 4, 0, 0), dev.search(p), ("identity", view, bs, sub))
        assert_bits(dev.search(p), wta(V, view, sub), ("search", view, bs, sub))
    p5 = params_of(wslib, view, 53 if bs == 33 else 51, 0, 64, "census5x5", True)        # the same bound for 5x5
    V5 = volume(L, R, view, p5.block_size, 0, 64, "census5x5")
    assert_bits(dev.sgm(p5, 4, 3, 20), sgm_from_volume(V5, view, 4, 3, 20, True), (view, p5.block_size))


# ---- the callers of the search dispatch ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair96():
    L, R = textured_pair(96, 200, 8, 96, black=True)
    want = {(v, c, s): wta(volume(L, R, v, 7, 0, 32, c), v, s) for v in VIEWS for c in COSTS for s in (False, True)}
    return L, R, want


@pytest.mark.parametrize("cost", COSTS)
def test_host_calls(wslib, gpu_ctx, pair96, cost):
    """ws_search_host (float32 and float64, with set_host_bands(4): a census call is never cut), ws_enqueue_host / ws_wait
    and ws_search_unrectified_host with identity homographies."""
    L, R, want = pair96
    try:
        for bands in (4, -1):
            gpu_ctx.set_host_bands(bands)
            for view in VIEWS:
                for sub in (False, True):
                    p = params_of(wslib, view, 7, 0, 32, cost, sub)
                    got = gpu_ctx.search(p, L, R)
                    assert got.dtype == np.float64 and got.tobytes() == want[view, cost, sub].tobytes(), (view, sub, bands)
                    assert_bits(gpu_ctx.search(p, L, R, dtype=np.float32), want[view, cost, sub], (view, sub, bands))
                    assert gpu_ctx.last_wire_format() == "float32"
                    assert gpu_ctx.last_launch()["kernel"] == MATCH_KERNEL
    finally:
        gpu_ctx.set_host_bands(-1)
    for view in VIEWS:
        p = params_of(wslib, view, 7, 0, 32, cost, True)
        outs = gpu_ctx.search_many(p, [(L, R), (L[:150], R[:150]), (L, R)])
        assert_bits(outs[0], want[view, cost, True], view)
        assert_bits(outs[2], want[view, cost, True], view)
        assert_bits(outs[1], wta(volume(L[:150], R[:150], view, 7, 0, 32, cost), view, True), view)
        got = gpu_ctx.search_unrectified(p, L, R, np.eye(3), np.eye(3))
        assert got.tobytes() == want[view, cost, True].tobytes(), view


@pytest.mark.parametrize("cost", COSTS)
def test_search_lr_against_the_reference_check(wslib, gpu_ctx, pair96, cost):
    L, R, want = pair96
    for fill in (False, True):
        p = params_of(wslib, "left", 7, 0, 32, cost)
        gl, gr = gpu_ctx.search_lr(p, L, R, 1.0, fill, dtype=np.float32)
        wl, wr, counts = lr_check(want["left", cost, False], want["right", cost, False], 1.0, fill)
        assert_bits(gl, wl, ("left", fill))
        assert_bits(gr, wr, ("right", fill))
        assert gpu_ctx.last_lr_counts() == counts


@pytest.mark.parametrize("cost", COSTS)
def test_batch_search_with_bands_requested(wslib, pair96, cost):
    """BatchSearch with bands=True: a batch with a census job is dealt as whole pairs, every map the reference's."""
    L, R, want = pair96
    with wslib.BatchSearch([0, 0]) as batch:
        for view in VIEWS:
            p = params_of(wslib, view, 7, 0, 32, cost)
            items, banded = batch.plan(p, [(L, R)] * 3, bands=True, min_rows=32)
            assert not banded and len(items) == 3
            for m in batch.search(p, [(L, R)] * 3, bands=True, min_rows=32):
                assert_bits(m, want[view, cost, False], view)
            sad = params_of(wslib, view, 7, 0, 32, "sad")
            maps = batch.search([sad, p, sad], [(L, R)] * 3, bands=True, min_rows=32)
            assert_bits(maps[1], want[view, cost, False], view)
            assert maps[0].tobytes() == maps[2].tobytes()


def test_two_census_kinds_back_to_back_on_two_streams(wslib, gpu_ctx, pair96):
    """The descriptor planes are the Searcher's scratch, 32 bits wide for 5x5 and 64 for 9x7: a search on another stream
    waits for the previous one's."""
    torch = _torch()
    L, R, want = pair96
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    tl, tr = dev_image(torch, L), dev_image(torch, R)
    torch.cuda.synchronize()
    outs = []
    for k in range(6):
        cost, view, s = COSTS[k % 2], VIEWS[(k // 2) % 2], (s1, s2)[k % 2]
        o = torch.zeros(L.shape[:2], dtype=torch.float32, device="cuda")
        gpu_ctx.search_device(params_of(wslib, view, 7, 0, 32, cost, True), tl, tr, o, stream=s.cuda_stream)
        outs.append((o, view, cost))
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    for o, view, cost in outs:
        assert_bits(o.cpu().numpy(), want[view, cost, True], (view, cost))


def test_profiling_brackets_the_match_kernel(wslib, gpu_ctx, pair96):
    torch = _torch()
    L, R, want = pair96
    dev = Device(wslib, gpu_ctx, L, R, "left")
    gpu_ctx.set_profiling(True)
    try:
        assert_bits(dev.search(params_of(wslib, "left", 7, 0, 32, "census9x7")), want["left", "census9x7", False], "profiled")
        assert gpu_ctx.last_kernel_ms() > 0
    finally:
        gpu_ctx.set_profiling(False)
    info = gpu_ctx.last_launch()
    plan = wslib.plan(params_of(wslib, "left", 7, 0, 32, "census9x7"), L.shape, R.shape)
    assert info == {"kernel": MATCH_KERNEL, "threads": plan["threads"], "workgroups": plan["tiles"] * plan["strips"],
                    "lds_bytes": plan["lds_bytes"]}
    torch.cuda.synchronize()


@pytest.mark.parametrize("cost", COSTS)
def test_cxx_facade(wslib, gpu_ctx, tmp_path, cost):
    """tests/cxx/census_driver.cpp: BlockSearch with a census cost on its left, right, checked and SGM methods, and
    wsamd::censusTransform."""
    exe = str(tmp_path / "census_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "census_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    L, R = textured_pair(90, 33, 6, 4, w2=85)
    (tmp_path / "l.raw").write_bytes(L.tobytes())
    (tmp_path / "r.raw").write_bytes(R.tobytes())
    maps, desc = tmp_path / "maps.raw", tmp_path / "desc.raw"
    subprocess.check_call([exe, str(tmp_path / "l.raw"), "90", "33", str(tmp_path / "r.raw"), "85", "33", str(wslib._COST[cost]),
                           "5", "1", "24", "3", "20", "8", str(maps), str(desc)])
    raw = np.frombuffer(maps.read_bytes(), dtype=np.float64)
    nl, nr = 33 * 90, 33 * 85
    assert raw.size == 3 * (nl + nr)
    parts = np.split(raw, [nl, nl + nr, 2 * nl + nr, 2 * nl + 2 * nr, 3 * nl + 2 * nr])
    left, right, cl, cr, sl, sr = [a.reshape(33, -1) for a in parts]
    VL, VR = volume(L, R, "left", 5, 1, 24, cost), volume(L, R, "right", 5, 1, 24, cost)
    assert_bits(left, wta(VL, "left"), "left")
    assert_bits(right, wta(VR, "right"), "right")
    wl, wr, _ = lr_check(wta(VL, "left"), wta(VR, "right"), 1.0, True)
    assert_bits(cl, wl, "checked left")
    assert_bits(cr, wr, "checked right")
    assert_bits(sl, sgm_from_volume(VL, "left", 8, 3, 20), "sgm left")
    assert_bits(sr, sgm_from_volume(VR, "right", 8, 3, 20), "sgm right")
    assert desc.read_bytes() == transform_np(L, cost).tobytes()


# ---- a whole map -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", COSTS)
def test_teddy_quarter_whole_map(wslib, gpu_ctx, cost):
    g = load_golden("teddy_quarter")
    want = wta(volume(g["left"], g["right"], "left", 7, 0, 64, cost), "left")
    got = gpu_ctx.search(params_of(wslib, "left", 7, 0, 64, cost), g["left"], g["right"], dtype=np.float32)
    assert_bits(got, want, cost)
    assert wslib.evaldisp(got, g["gt"], g["mask"], 2.0, 64.0) == wslib.evaldisp(want, g["gt"], g["mask"], 2.0, 64.0)
    assert gpu_ctx.last_launch()["kernel"] == MATCH_KERNEL
