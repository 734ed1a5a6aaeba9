"""The left-right consistency check on the device (ws_lr_check_device, ws_search_lr_host / _device, ws_last_lr_counts,
BlockSearch.computeDisparityMapsChecked): every map bit for bit and every count equal to tests/lr_ref.py -- on seeded
random maps of awkward sizes, on the oracle's maps of the searches, on two Middlebury pairs, and through the pipeline
of main.cpp:40-64 into the mesh."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from lr_ref import FAILED, lr_check, lr_states
from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

WS_ERR_ARG = -1
CALIB = os.path.join(ROOT, "tests", "golden", "teddy_calib.txt")
VALUES = np.array([0, -0.0, 1, 2, 3, 5, 2.5, 3.5, -1, -2, 1.25, np.nan, np.inf, -np.inf], dtype=np.float32)


def _torch():
    import torch
    return torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, bad[:5].tolist(), [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:3]])


def random_maps(rng, hl, wl, hr, wr):
    """Disparities of a consistent scene (right(y, x) = d where left(y, x + d) = d) with every kind of value mixed in."""
    left = rng.integers(0, 6, size=(hl, wl)).astype(np.float32)
    right = np.zeros((hr, wr), dtype=np.float32)
    for y in range(min(hl, hr)):
        xs = np.arange(wl)
        p = xs - left[y].astype(np.int64)
        ok = (p >= 0) & (p < wr)
        right[y, p[ok]] = left[y, ok]
    for m in (left, right):
        noise = rng.random(m.shape) < 0.3
        m[noise] = rng.choice(VALUES, size=int(noise.sum()))
    return left, right


def padded(torch, a, pad, fill=7.0):
    """a (h x w float32) in a CUDA tensor whose rows are w + pad floats apart; the padding holds `fill`."""
    h, w = a.shape
    t = torch.full((h, w + pad), fill, dtype=torch.float32, device="cuda")
    t[:, :w] = torch.from_numpy(np.ascontiguousarray(a))
    return t[:, :w]


def run_check(ctx, left, right, max_diff, fill, pads=(0, 0, 0, 0), stream=None):
    torch = _torch()
    tl, tr = padded(torch, left, pads[0]), padded(torch, right, pads[1])
    ol = padded(torch, np.full(left.shape, 9.0, np.float32), pads[2], fill=-5.0)
    orr = padded(torch, np.full(right.shape, 9.0, np.float32), pads[3], fill=-5.0)
    torch.cuda.synchronize()
    ctx.lr_check_device(tl, tr, ol, orr, max_diff, fill, stream=stream)
    counts = ctx.last_lr_counts()
    torch.cuda.synchronize()
    for t, pad in ((ol, pads[2]), (orr, pads[3])):  # the row padding of an output is never written
        if pad:
            full = t.as_strided((t.shape[0], t.stride(0)), (t.stride(0), 1))
            assert bool((full[:, t.shape[1]:] == -5.0).all())
    return ol.cpu().numpy(), orr.cpu().numpy(), counts


WIDTHS = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5000]
HEIGHTS = [1, 2, 17]
MAX_DIFFS = [0.0, 0.5, 1.0, 3.0, np.inf]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_check_on_random_maps(gpu_ctx, w, h):
    rng = np.random.default_rng(1000 * w + h)
    left, right = random_maps(rng, h, w, h, w)
    for i, fill in enumerate((False, True)):
        md = MAX_DIFFS[(w + h + i) % len(MAX_DIFFS)]
        want_l, want_r, want_c = lr_check(left, right, md, fill)
        got_l, got_r, got_c = run_check(gpu_ctx, left, right, md, fill)
        assert_bits(got_l, want_l, ("left", w, h, md, fill))
        assert_bits(got_r, want_r, ("right", w, h, md, fill))
        assert got_c == want_c


@pytest.mark.parametrize("sizes", [((17, 300), (13, 290)), ((5, 4097), (9, 4000)), ((2, 64), (2, 65)), ((1, 5000), (3, 1)),
                                   ((17, 1), (1, 257))])
@pytest.mark.parametrize("pads", [(0, 0, 0, 0), (3, 64, 1, 5)])
def test_check_unequal_sizes_and_padded_strides(gpu_ctx, sizes, pads):
    (hl, wl), (hr, wr) = sizes
    rng = np.random.default_rng(hl * 7 + wl + wr)
    left, right = random_maps(rng, hl, wl, hr, wr)
    for md in MAX_DIFFS:
        for fill in (False, True):
            want_l, want_r, want_c = lr_check(left, right, md, fill)
            got_l, got_r, got_c = run_check(gpu_ctx, left, right, md, fill, pads)
            assert_bits(got_l, want_l, ("left", sizes, md, fill))
            assert_bits(got_r, want_r, ("right", sizes, md, fill))
            assert got_c == want_c


def test_check_argument_errors(wslib, gpu_ctx):
    torch = _torch()
    a = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    b = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    ol = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    orr = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    for md in (np.nan, -1.0, -0.5):
        with pytest.raises(wslib.WsError) as e:
            gpu_ctx.lr_check_device(a, b, ol, orr, md)
        assert e.value.code == WS_ERR_ARG
    six = torch.zeros((6, 8), dtype=torch.float32, device="cuda")
    for outs in ((a, orr), (ol, b), (ol, ol), (six[:4], six[2:])):
        with pytest.raises(wslib.WsError) as e:
            gpu_ctx.lr_check_device(a, b, outs[0], outs[1], 1.0)
        assert e.value.code == WS_ERR_ARG
    big = torch.zeros((4, 20), dtype=torch.float32, device="cuda")  # the outputs' rows interleave: their ranges overlap
    with pytest.raises(wslib.WsError) as e:
        gpu_ctx.lr_check_device(a, b, big[:, :8], big[:, 8:16], 1.0)
    assert e.value.code == WS_ERR_ARG
    lib, h = wslib.load_library(), gpu_ctx._h
    lr = wslib.lr_params(1.0)
    p_a, p_b, p_l, p_r = a.data_ptr(), b.data_ptr(), ol.data_ptr(), orr.data_ptr()
    assert lib.ws_lr_check_device(h, None, 8, 4, 8, p_b, 8, 4, 8, ctypes.byref(lr), p_l, 8, p_r, 8, None) == WS_ERR_ARG
    assert lib.ws_lr_check_device(h, p_a, 8, 4, 8, p_b, 8, 4, 8, None, p_l, 8, p_r, 8, None) == WS_ERR_ARG
    assert lib.ws_lr_check_device(h, p_a, 8, 4, 8, p_b, 8, 4, 8, ctypes.byref(lr), None, 8, p_r, 8, None) == WS_ERR_ARG
    assert lib.ws_lr_check_device(h, p_a, 8, 4, 7, p_b, 8, 4, 8, ctypes.byref(lr), p_l, 8, p_r, 8, None) == WS_ERR_ARG
    assert lib.ws_lr_check_device(h, p_a, 8, 4, 8, p_b, 8, 4, 8, wslib._LrParams(1.0, 2), p_l, 8, p_r, 8, None) == WS_ERR_ARG
    assert lib.ws_last_lr_counts(h, None) == WS_ERR_ARG
    img = wslib._Image(None, 8, 4, 24)
    params = wslib.make_params(wslib.VIEW_LEFT, 5, 0, 4)
    out = np.zeros((4, 8), np.float32)
    assert lib.ws_search_lr_host(h, ctypes.byref(params), ctypes.byref(img), ctypes.byref(img), ctypes.byref(lr),
                                 out.ctypes.data, 8, out.ctypes.data, 8, 0) == WS_ERR_ARG
    # the check must still work after the refusals
    want_l, want_r, want_c = lr_check(np.ones((4, 8), np.float32), np.ones((4, 8), np.float32), 1.0)
    got_l, got_r, got_c = run_check(gpu_ctx, np.ones((4, 8), np.float32), np.ones((4, 8), np.float32), 1.0, False)
    assert_bits(got_l, want_l, "left")
    assert got_c == want_c


# (label, search kwargs for make_params, oracle of the left map, oracle of the right map)
def _oracle_maps(oracle, left, right, bs, mind, maxd, smooth=1.0, cost="ssd", var_block=False, thres=19.0, subpixel=False):
    sp = "float32" if subpixel else False
    dl = oracle.fast_left(left, right, bs, mind, maxd, smooth=smooth, cost=cost, subpixel=sp)
    if var_block:
        dr = oracle.block_right(left, right, bs, mind, maxd, smooth=smooth, var_block=True, thres=thres, cost=cost)
    else:
        dr = oracle.fast_right(left, right, bs, mind, maxd, smooth=smooth, cost=cost, subpixel=sp)
    return dl.astype(np.float32), dr.astype(np.float32)


SEARCH_CASES = [
    dict(bs=5, cost="ssd"), dict(bs=7, cost="sad"), dict(bs=17, cost="ssd"), dict(bs=7, cost="ssd", smooth=0.9),
    dict(bs=5, cost="sad", smooth=0.9), dict(bs=17, cost="ssd", smooth=0.9), dict(bs=5, cost="ssd", var_block=True),
    dict(bs=7, cost="ssd", var_block=True, thres=10.0, smooth=0.9), dict(bs=7, cost="ssd", subpixel=True),
    dict(bs=9, cost="sad", subpixel=True), dict(bs=7, cost="ssd", mind=4), dict(bs=5, cost="sad", mind=3, smooth=0.9),
]


@pytest.mark.parametrize("case", range(len(SEARCH_CASES)))
@pytest.mark.parametrize("sizes", ["equal", "unequal"])
def test_search_lr_host_against_the_oracle(wslib, gpu_ctx, oracle, case, sizes):
    c = dict(SEARCH_CASES[case])
    bs, cost, smooth, mind = c.pop("bs"), c.pop("cost"), c.pop("smooth", 1.0), c.pop("mind", 0)
    maxd = 24
    if sizes == "equal":
        left, right, _ = make_pair(160, 60, maxd, seed=40 + case)
    else:
        left, right, _ = make_pair(170, 60, maxd, seed=40 + case, right_width=150)
    dl, dr = _oracle_maps(oracle, left, right, bs, mind, maxd, smooth, cost, **c)
    for md, fill in ((1.0, False), (0.0, True), (np.inf, False), (2.5, True)):
        want_l, want_r, want_c = lr_check(dl, dr, md, fill)
        p = wslib.make_params(wslib.VIEW_RIGHT, bs, mind, maxd, smooth, cost, c.get("var_block", False), c.get("thres", 19.0),
                              c.get("subpixel", False))
        for dtype in (np.float32, np.float64):
            got_l, got_r = gpu_ctx.search_lr(p, left, right, md, fill, dtype=dtype)
            assert got_l.dtype == dtype and got_r.dtype == dtype
            assert_bits(got_l.astype(np.float32), want_l, ("left", c, md, fill, dtype))
            assert_bits(got_r.astype(np.float32), want_r, ("right", c, md, fill, dtype))
            if dtype == np.float64:
                assert np.array_equal(got_l, want_l.astype(np.float64), equal_nan=True)
            assert gpu_ctx.last_lr_counts() == want_c


def test_search_lr_refuses_what_search_host_refuses(wslib, gpu_ctx):
    left, right, _ = make_pair(120, 40, 16, seed=5)
    La, Li = wslib._host_image(left)
    Ra, Ri = wslib._host_image(right)
    lib, h = wslib.load_library(), gpu_ctx._h
    lr = wslib.lr_params(1.0)
    cases = [dict(block_size=6), dict(block_size=64), dict(subpixel=True, smooth_factor=0.9), dict(subpixel=True, var_block=True),
             dict(min_disparity=-2), dict(cost=5), dict(smooth_factor=float("nan")), dict(var_block=True, thres=float("nan")),
             dict(block_size=4, min_disparity=-1)]
    for kw in cases:
        p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 16)
        for k, v in kw.items():
            setattr(p, k, v)
        codes = []
        for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT):
            p.view = view
            out = np.zeros((40, 120), np.float64)
            codes.append(lib.ws_search_host(h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), out.ctypes.data, 120, 1))
        want = next((c for c in codes if c != 0), 0)
        assert want != 0, kw
        for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT, wslib.VIEW_LINEAR):  # p.view is ignored
            p.view = view
            ol, orr = np.zeros((40, 120), np.float64), np.zeros((40, 120), np.float64)
            got = lib.ws_search_lr_host(h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), ctypes.byref(lr),
                                        ol.ctypes.data, 120, orr.ctypes.data, 120, 1)
            assert got == want, (kw, view, got, codes)


def test_search_lr_device_on_a_torch_stream(wslib, gpu_ctx, oracle):
    torch = _torch()
    left, right, _ = make_pair(300, 90, 40, seed=77, right_width=280)
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 40, 0.9, "ssd")
    dl, dr = _oracle_maps(oracle, left, right, 7, 0, 40, 0.9, "ssd")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tl = torch.from_numpy(left).cuda()
        tr = torch.from_numpy(right).cuda()
        ol = torch.full((90, 300), -5.0, dtype=torch.float32, device="cuda")
        orr = torch.full((90, 280 + 3), -5.0, dtype=torch.float32, device="cuda")[:, :280]
        for md, fill in ((1.0, True), (0.0, False)):
            want_l, want_r, want_c = lr_check(dl, dr, md, fill)
            gpu_ctx.search_lr_device(p, tl, tr, ol, orr, md, fill, stream=s.cuda_stream, check=True)
            assert gpu_ctx.last_lr_counts() == want_c
            s.synchronize()
            assert_bits(ol.cpu().numpy(), want_l, ("left", md, fill))
            assert_bits(orr.cpu().numpy(), want_r, ("right", md, fill))
            assert bool((orr.as_strided((90, 283), (283, 1))[:, 280:] == -5.0).all())
    # the same maps from the host call
    got_l, got_r = gpu_ctx.search_lr(p, left, right, 0.0, False, dtype=np.float32)
    assert_bits(got_l, want_l, "host left")
    assert_bits(got_r, want_r, "host right")


def scene_maps(rng, h, w):
    """Integer disparity maps of a consistent scene (one disparity per 64-column block of a row; right(y, x - d) = d),
    then a tenth of each map's pixels moved off by 3 .. 6: about a fifth of the pixels fail at max_diff 1."""
    left = np.repeat(rng.integers(1, 9, size=(h, (w + 63) // 64)), 64, axis=1)[:, :w].astype(np.float32)
    right = np.zeros((h, w), dtype=np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    p = xs - left.astype(np.int64)
    right[ys[p >= 0], p[p >= 0]] = left[p >= 0]
    for m in (left, right):
        off = (rng.random(m.shape) < 0.1) & (m != 0)
        m[off] += rng.integers(3, 7, size=int(off.sum())).astype(np.float32)
    return left, right


def test_two_streams_share_the_check_scratch_without_a_host_wait(wslib):
    """A large check on stream A, at once a small one on stream B, then A again and B again, on one context with the
    background fill (counters and state plane shared), the host waiting only at the end: each call's kernels must wait
    for those of the call before it (the check's scratch lease).  A guard, not a proof: it cannot show that the wait
    is there, only catch some ways of losing it."""
    torch = _torch()
    rng = np.random.default_rng(1024)
    a, b = scene_maps(rng, 512, 1024), scene_maps(rng, 40, 96)
    want_a, want_b = lr_check(*a, 1.0, True), lr_check(*b, 1.0, True)
    assert 0.1 < want_a[2][0] / a[0].size < 0.3 and 0.1 < want_a[2][1] / a[1].size < 0.3, want_a[2]
    with wslib.WindowSearch(0) as ctx:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ta, tb = (tuple(torch.from_numpy(x).cuda() for x in m) for m in (a, b))
        calls = [(t, want, s, tuple(torch.full_like(x, float("nan")) for x in t))
                 for t, want, s in ((ta, want_a, sa), (tb, want_b, sb), (ta, want_a, sa), (tb, want_b, sb))]
        torch.cuda.synchronize()                 # the maps and the NaN outputs are in place; from here on no host wait
        for t, _, s, outs in calls:
            ctx.lr_check_device(*t, *outs, 1.0, True, stream=s.cuda_stream)
        counts = ctx.last_lr_counts()            # (waits for the last check alone)
        torch.cuda.synchronize()
        assert counts == want_b[2]
        for (_, want, _, outs), what in zip(calls, ("A", "B", "A again", "B again")):
            assert_bits(outs[0].cpu().numpy(), want[0], (what, "left"))
            assert_bits(outs[1].cpu().numpy(), want[1], (what, "right"))


def test_the_cxx_facade_returns_the_checked_maps(wslib, gpu_ctx, oracle, tmp_path):
    left, right, _ = make_pair(140, 50, 20, seed=9, right_width=130)
    exe = str(tmp_path / "lr_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "lr_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    lp, rp, op = str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(tmp_path / "o.raw")
    left.tofile(lp)
    right.tofile(rp)
    subprocess.check_call([exe, lp, "140", "50", rp, "130", "50", "9", "0", "20", "0.9", "1.5", "1", op], timeout=300)
    got = np.fromfile(op, dtype=np.float64)
    dl, dr = _oracle_maps(oracle, left, right, 9, 0, 20, 0.9)
    want_l, want_r, _ = lr_check(dl, dr, 1.5, True)
    assert np.array_equal(got[:140 * 50].reshape(50, 140), want_l.astype(np.float64))
    assert np.array_equal(got[140 * 50:].reshape(50, 130), want_r.astype(np.float64))
    # the Python facade
    ml, mr = wslib.BlockSearch(left, right, 9, 0, 20, context=gpu_ctx).computeDisparityMapsChecked(0.9, 1.5, True)
    assert np.array_equal(ml, want_l.astype(np.float64)) and np.array_equal(mr, want_r.astype(np.float64))


# Worked out on the CPU from the oracle's maps (fast_left / fast_right, 7 x 7 SSD, D = ndisp = 128) and tests/lr_ref.py:
# (failed left, failed right, evaldisp of the unchecked left map (n, bad, invalid), of the checked one (n, bad, invalid))
MIDDLEBURY = {
    "teddyH_pair": (226961, 221071, (586756, 26.693037033081055, 1.2154967784881592), (586756, 9.557294845581055, 28.650068283081055)),
    "artL_pair": (272706, 269168, (291686, 72.24446868896484, 1.764225959777832), (291686, 15.834493637084961, 68.43729400634766)),
}


@pytest.mark.parametrize("name", sorted(MIDDLEBURY))
def test_middlebury_bad2_drops_on_the_checked_pixels(wslib, gpu_ctx, oracle, name):
    g = load_golden(name)
    nd = int(g["ndisp"])
    fail_l, fail_r, raw_e, chk_e = MIDDLEBURY[name]
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, nd, 1.0, "ssd")
    got_l, got_r = gpu_ctx.search_lr(p, g["left"], g["right"], 1.0, False, dtype=np.float32)
    dl, dr = _oracle_maps(oracle, g["left"], g["right"], 7, 0, nd)
    want_l, want_r, want_c = lr_check(dl, dr, 1.0)
    assert_bits(got_l, want_l, "left")
    assert_bits(got_r, want_r, "right")
    assert gpu_ctx.last_lr_counts() == want_c == (fail_l, fail_r)
    raw = wslib.evaldisp(dl, g["gt"], g["mask"], 2.0, float(nd))
    chk = wslib.evaldisp(got_l, g["gt"], g["mask"], 2.0, float(nd))
    assert chk == oracle.evaldisp(want_l, g["gt"], g["mask"], 2.0, float(nd))
    assert (raw["n"], raw["bad"], raw["invalid"]) == pytest.approx(raw_e, abs=1e-9)
    assert (chk["n"], chk["bad"], chk["invalid"]) == pytest.approx(chk_e, abs=1e-9)
    # bad-2.0 among the pixels that keep a value (evaldisp counts d == 0 as invalid, not bad)
    assert chk["bad"] / (100.0 - chk["invalid"]) < raw["bad"] / (100.0 - raw["invalid"])


def test_pipeline_mesh_of_the_checked_right_map(wslib, gpu_ctx, oracle, tmp_path):
    """main.cpp:40-64 with the checked right map: computeDisparityMapRight(17, 0, 200, 0.9), then depth and the mesh.
    Every failed pixel is an invalid vertex ("0 0 0 ...") that no face uses."""
    left, right, _ = make_pair(240, 150, 120, seed=31)
    p = wslib.make_params(wslib.VIEW_RIGHT, 17, 0, 200, 0.9, "ssd")
    _, got_r = gpu_ctx.search_lr(p, left, right, 1.0, False, dtype=np.float32)
    dl, dr = _oracle_maps(oracle, left, right, 17, 0, 200, 0.9)
    _, want_r, _ = lr_check(dl, dr, 1.0)
    assert_bits(got_r, want_r, "right")
    K = wslib.read_calib(CALIB)["cam1"]
    f, b, thr = 3000.0, 1.0, 1.0
    depth = gpu_ctx.convert_disparity_to_depth(got_r, f, b)
    path = str(tmp_path / "checked.off")
    gpu_ctx.reconstruction(depth, K, right, thr, path)
    with open(path, "rb") as fh:
        got = fh.read()
    pos, col = oracle.back_project(oracle.convert_disparity_to_depth(want_r, f, b), K, right)
    want = oracle.mesh_off_text(pos, col, thr)
    assert got == (want.encode() if isinstance(want, str) else want)
    lines = got.decode().split("\n")
    nv, nf = map(int, lines[1].split()[:2])
    verts, faces = lines[2:2 + nv], lines[2 + nv:2 + nv + nf]
    _, st_r = lr_states(dl, dr, 1.0)
    failed = np.flatnonzero(st_r.reshape(-1) == FAILED)
    assert failed.size > 0 and nf > 0
    assert all(verts[i].startswith("0 0 0 ") for i in failed)
    used = np.zeros(nv, dtype=bool)
    used[np.array([list(map(int, ln.split()[1:4])) for ln in faces]).reshape(-1)] = True
    assert not used[failed].any()
