"""The pair call on the device (ws_search_pair_device / _host, BlockSearch::computeDisparityMapsCheckedSGM): both views'
maps from one volume, whole maps as float32 bits against tests/pair_ref.py -- on the tiny seeds, the periodic pairs and
staircases of tests/pair_inputs.py, on images of unequal sizes, at every storage width of the volume, on both sides of
the span switch of the diagonal winner kernel, with the uniqueness ratio, with the left-right check, through the host
form and the C++ facade, and across streams that share the scratch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lr_ref
from conftest import ROOT
from pair_inputs import PERIODIC, STAIRCASES, case_sums, kernel_constant, periodic_case, staircase_case
from pair_ref import derived_np, other_shape, pair_np
from sgm_inputs import GEOMETRIES, geometry_case
from test_gpu_sgm import assert_bits, dev_image, params_of
from test_pair_reference import tiny_views
from test_subpixel_reference import shifted_pair
from unique_ref import unique_from_sums

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


class Pair:
    """A pair on the device, and pair calls on it into fresh NaN-filled maps with padded rows."""

    def __init__(self, ctx, L, R, pad=0):
        torch = _torch()
        self.ctx, self.pad = ctx, pad
        self.tl, self.tr = dev_image(torch, L, pad), dev_image(torch, R, pad)
        self.lshape, self.rshape = L.shape[:2], R.shape[:2]

    def planes(self):
        torch = _torch()
        return [torch.full((h, w + pad), float("nan"), dtype=torch.float32, device="cuda")
                for (h, w), pad in ((self.lshape, self.pad), (self.rshape, 2 * self.pad))]

    def host(self, planes):
        res = []
        for t, (h, w) in zip(planes, (self.lshape, self.rshape)):
            a = t.cpu().numpy()
            assert np.isnan(a[:, w:]).all(), "the padding of the rows was written"
            res.append(a[:, :w])
        return res

    def run(self, params, sgm=None, ratio=None, lr=None, stream=None):
        """(left map, right map) of one call"""
        ol, orr = self.planes()
        s = stream.cuda_stream if stream is not None else None
        self.ctx.search_pair_device(params, self.tl, self.tr, ol[:, :self.lshape[1]], orr[:, :self.rshape[1]], sgm, ratio,
                                    None if lr is None else lr[0], bool(lr and lr[1]), stream=s)
        _torch().cuda.synchronize()
        return self.host((ol, orr))

    def check_alone(self, left, right, lr):
        """ws_lr_check_device on two maps (numpy) -> (left, right, counts)"""
        torch = _torch()
        a, b = torch.from_numpy(np.ascontiguousarray(left)).cuda(), torch.from_numpy(np.ascontiguousarray(right)).cuda()
        ol, orr = self.planes()
        self.ctx.lr_check_device(a, b, ol[:, :self.lshape[1]], orr[:, :self.rshape[1]], lr[0], lr[1])
        counts = self.ctx.last_lr_counts()
        torch.cuda.synchronize()
        return self.host((ol, orr)) + [counts]


def check(wslib, ctx, L, R, view, bs, mind, maxd, cost, sgm, sub=False, ratio=None, lr=None, pad=0, pair=None):
    """The raw maps of a call against the reference and, with lr, the checked ones and the counts too."""
    pair = pair or Pair(ctx, L, R, pad)
    p = params_of(wslib, view, bs, mind, maxd, cost, sub)
    want = pair_np(L, R, view, bs, mind, maxd, cost, sgm, ratio, sub, lr)
    what = (view, bs, mind, maxd, cost, sgm, sub, ratio, L.shape, R.shape)
    left, right = pair.run(p, sgm, ratio)
    assert_bits(left, want["left"], ("left",) + what)
    assert_bits(right, want["right"], ("right",) + what)
    if ratio is not None:
        assert ctx.last_unique_counts() == want["unique_counts"], what
    if lr is not None:
        cl, cr = pair.run(p, sgm, ratio, lr)
        counts = ctx.last_lr_counts()
        assert_bits(cl, want["checked_left"], ("checked left", lr) + what)
        assert_bits(cr, want["checked_right"], ("checked right", lr) + what)
        assert counts == want["lr_counts"], (what, counts, want["lr_counts"])
    return want


@pytest.mark.parametrize("first", range(0, 48, 8))
def test_tiny_seeds(wslib, gpu_ctx, first):
    for seed in range(first, first + 8):
        sub = seed % 3 == 1
        for L, R, view, bs, mind, maxd, cost, paths, p1, p2 in tiny_views(seed):
            pair = Pair(gpu_ctx, L, R, pad=seed % 2)
            check(wslib, gpu_ctx, L, R, view, bs, mind, maxd, cost, (paths, p1, p2), sub, lr=(1.0, seed % 2 == 0), pair=pair)
            check(wslib, gpu_ctx, L, R, view, bs, mind, maxd, cost, None, sub, pair=pair)


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("name", sorted(PERIODIC))
def test_periodic_pairs(wslib, gpu_ctx, name, view):
    """Exact ties among a derived pixel's candidates: the tie rule alone decides (tests/test_pair_inputs.py)."""
    L, R, maxd = periodic_case(name)
    pair = Pair(gpu_ctx, L, R)
    for sgm in (None, (4, 0, 0)):
        check(wslib, gpu_ctx, L, R, view, 3, 0, maxd, "sad", sgm, pair=pair)


@pytest.mark.parametrize("name", sorted(STAIRCASES))
def test_staircases(wslib, gpu_ctx, name):
    """Derived winners in every 64-lane chunk of a curve, up to the 2048 disparities a call takes."""
    L, R, (view, bs, mind, maxd, cost), sgm, nd = staircase_case(name)
    V, S = case_sums(L, R, view, bs, mind, maxd, cost, sgm)
    p = params_of(wslib, view, bs, mind, maxd, cost)
    left, right = Pair(gpu_ctx, L, R, pad=1).run(p, sgm)
    base = unique_from_sums(V, S, view, 0)["map"]
    der = derived_np(S, V[1], view, other_shape(L, R, view))
    assert_bits(left if view == "left" else right, base, (name, "base"))
    assert_bits(right if view == "left" else left, der, (name, "derived"))


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_geometry(wslib, gpu_ctx, name):
    """A right image wider, taller, or both: derived rows beyond the base map's rows, columns nobody offers to."""
    maxd = 12
    L, R, view, mind = geometry_case(name, 61, 17, maxd)
    for sgm in (None, (4, 60, 900)):
        want = check(wslib, gpu_ctx, L, R, view, 5, mind, maxd, "ssd", sgm, True, lr=(1.0, True), pad=2)
        der = want["right" if view == "left" else "left"]
        assert (der == 0).sum() > 20 and (der > 0).sum() > 200


def test_smaller_right_image_min_disparity_and_black_runs(wslib, gpu_ctx):
    L, R = shifted_pair(90, 33, 7, 4)
    Rs = R[:29, :83].copy()
    for view, mind in (("left", 0), ("right", 0), ("right", 3)):
        check(wslib, gpu_ctx, L, Rs, view, 5, mind, 24, "sad", (8, 30, 300), lr=(1.0, False), pad=3)
        check(wslib, gpu_ctx, L, Rs, view, 5, mind, 24, "sad", None, lr=(2.0, True))
    Lb, Rb = L.copy(), R.copy()
    Lb[10:14, 20:60] = 0
    Rb[15:25, 40:48] = 0
    Rb[3, :] = 0
    for view, mind in (("left", 0), ("right", 3)):
        want = check(wslib, gpu_ctx, Lb, Rb, view, 3, mind, 30, "ssd", (4, 100, 1000), lr=(1.0, True))
        assert (want["left" if view == "left" else "right"] == 0).sum() > 100


@pytest.mark.parametrize("what,cost,bs,sgm,widths", [
    ("cost16", "sad", 3, None, (1, 0)), ("cost32", "ssd", 7, None, (0, 0)), ("sum32", "ssd", 5, (8, 200, 1800), (0, 0)),
    ("sum64", "sad", 3, (8, 7, 2 ** 31 - 1), (1, 1)), ("census", "census5x5", 5, (8, 3, 20), (1, 0))])
def test_storage_widths(wslib, gpu_ctx, what, cost, bs, sgm, widths):
    from sgm_ref import BIG
    L, R = shifted_pair(140, 31, 13, 7)
    for view, mind in (("left", 0), ("right", 1)):
        V, S = case_sums(L, R, view, bs, mind, 70, cost, sgm)
        cmax = {"sad": 765, "ssd": 195075, "census5x5": 24}[cost] * bs * bs
        assert (cmax <= 0xffff) == bool(widths[0])
        if sgm:
            assert (sgm[0] * (cmax + sgm[2]) > 0xffffffff) == bool(widths[1])
            if what == "sum32":
                assert int(S[S < BIG].max()) > 0xffff
        check(wslib, gpu_ctx, L, R, view, bs, mind, 70, cost, sgm, lr=(1.0, False))


def span_widths():
    T, W = kernel_constant("kPairSpan"), kernel_constant("kPairSwitchWidth")
    return [W - 1, W, W + 1, 2 * T + 1]


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("i", range(4))
def test_the_span_switch(wslib, gpu_ctx, i, view):
    """Derived rows of one span, of two with one column in the second, and of three; wherever a row has a seam, winners
    in the columns on both sides of it."""
    w = span_widths()[i]
    T = kernel_constant("kPairSpan")
    L, R = shifted_pair(w, 3, 3, 60 + i)
    mind = 1 if view == "right" else 0
    for sgm in ((4, 5, 40), None):
        # (three rows: the left view's full windows fit with block size 1 only; the right view's clipped ones need 3)
        want = check(wslib, gpu_ctx, L, R, view, 1 if view == "left" else 3, mind, mind + 8 if view == "right" else 8, "sad", sgm)
        der = want["right" if view == "left" else "left"]
        # winners in every column next to every seam; nobody offers to the last derived column (left base: d >= 1; right
        # base: x + d stays left of the clipped window's right edge)
        for seam in range(T, w, T):
            assert (der[:, seam - 8:min(w - 1, seam + 8)] > 0).all(), (w, view, seam)
            assert (der[:, w - 1] == 0).all()


@pytest.mark.parametrize("view", ["left", "right"])
def test_uniqueness(wslib, gpu_ctx, view):
    """The base map is ws_search_unique_device's, the counts its counts; the derived map does not see the ratio."""
    torch = _torch()
    L, R = shifted_pair(140, 37, 13, 7)
    mind = 1 if view == "right" else 0
    p = params_of(wslib, view, 5, mind, 40, "ssd", True)
    pair = Pair(gpu_ctx, L, R)
    for sgm in (None, (8, 300, 3000)):
        want = check(wslib, gpu_ctx, L, R, view, 5, mind, 40, "ssd", sgm, True, ratio=15, lr=(1.0, True), pair=pair)
        assert want["unique_counts"][0] > 20
        left, right = pair.run(p, sgm, 15)
        counts = gpu_ctx.last_unique_counts()
        h, w = pair.lshape if view == "left" else pair.rshape
        alone = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
        gpu_ctx.search_unique_device(p, pair.tl, pair.tr, alone, 15, sgm)
        assert gpu_ctx.last_unique_counts() == counts == want["unique_counts"]
        torch.cuda.synchronize()
        assert_bits(left if view == "left" else right, alone.cpu().numpy(), (view, sgm, "base"))
        plain = pair.run(p, sgm)
        assert_bits((right, left)[view == "right"], (plain[1], plain[0])[view == "right"], (view, sgm, "derived"))
        assert ((left if view == "left" else right) != (plain[0] if view == "left" else plain[1])).sum() > 20


@pytest.mark.parametrize("fill", [False, True])
def test_the_check_is_the_check_of_the_raw_maps(wslib, gpu_ctx, fill):
    L, R = shifted_pair(150, 47, 9, 3)
    L = L.copy()
    L[20:24, 30:70] = 0
    for view, sgm in (("left", (8, 300, 3000)), ("right", None)):
        p = params_of(wslib, view, 5, 0, 48, "ssd", True)
        pair = Pair(gpu_ctx, L, R, pad=5)
        raw = pair.run(p, sgm)
        got = pair.run(p, sgm, lr=(1.5, fill))
        counts = gpu_ctx.last_lr_counts()
        cl, cr, counts2 = pair.check_alone(raw[0], raw[1], (1.5, fill))
        assert_bits(got[0], cl, (view, "left"))
        assert_bits(got[1], cr, (view, "right"))
        rl, rr, rcounts = lr_ref.lr_check(raw[0], raw[1], 1.5, fill)
        assert_bits(got[0], rl, (view, "left, reference"))
        assert_bits(got[1], rr, (view, "right, reference"))
        assert counts == counts2 == rcounts and min(counts) > 50


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_host_form(wslib, gpu_ctx, dtype):
    L, R = shifted_pair(150, 47, 9, 3)
    R = R[:45, :141].copy()
    lib = wslib.load_library()
    code = wslib.OUT_F64 if dtype == np.float64 else wslib.OUT_F32
    for view, sgm, ratio, lr in (("left", (8, 300, 3000), None, (1.0, True)), ("right", None, 25, None), ("left", (4, 9, 90), 10, (1.0, False))):
        p = params_of(wslib, view, 5, 0, 48, "ssd", True)
        want = pair_np(L, R, view, 5, 0, 48, "ssd", sgm, ratio, True, lr)
        wl, wr = (want["checked_left"], want["checked_right"]) if lr else (want["left"], want["right"])
        gl, gr = gpu_ctx.search_pair(p, L, R, sgm, ratio, None if lr is None else lr[0], bool(lr and lr[1]), dtype=dtype)
        assert gl.dtype == dtype and gr.dtype == dtype
        assert gpu_ctx.last_host_paths() == ("staged",) * 3
        assert_bits(gl.astype(np.float32), wl, (view, "host left"))
        assert_bits(gr.astype(np.float32), wr, (view, "host right"))
        assert gl.astype(np.float32).astype(dtype).tobytes() == gl.tobytes()
        if lr:
            assert gpu_ctx.last_lr_counts() == want["lr_counts"]
        if ratio is not None:
            assert gpu_ctx.last_unique_counts() == want["unique_counts"]
        # padded strides, through the C-ABI itself
        pl, pr = np.full((47, 150 + 9), np.nan, dtype), np.full((45, 141 + 4), np.nan, dtype)
        Li, Ri = wslib._image_struct(L), wslib._image_struct(R)
        sp = None if sgm is None else wslib.sgm_params(*sgm)
        uq = None if ratio is None else wslib.unique_params(ratio)
        lrp = None if lr is None else wslib.lr_params(*lr)
        ref = lambda s: None if s is None else ctypes.byref(s)
        rc = lib.ws_search_pair_host(gpu_ctx._h, ctypes.byref(p), ref(sp), ref(uq), ref(lrp), ctypes.byref(Li), ctypes.byref(Ri),
                                     pl.ctypes.data, pl.shape[1], pr.ctypes.data, pr.shape[1], code)
        assert rc == 0
        assert np.isnan(pl[:, 150:]).all() and np.isnan(pr[:, 141:]).all()
        assert pl[:, :150].tobytes() == gl.tobytes() and pr[:, :141].tobytes() == gr.tobytes()


def test_shared_scratch_across_streams(wslib):
    """A pair call on stream A, an SGM call that needs more scratch on stream B, the pair call again, on a context of
    their own (its scratch starts empty); the host waits only at the end."""
    torch = _torch()
    from sgm_ref import sgm_np
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    L, R = shifted_pair(120, 40, 9, 9)
    L2, R2 = shifted_pair(400, 60, 30, 10)
    p = params_of(wslib, "left", 5, 0, 32, "sad", True)
    p2 = params_of(wslib, "left", 5, 0, 96, "ssd")
    assert wslib.sgm_scratch_bytes(p2, L2, R2, 8, 40, 200) > 4 * wslib.sgm_scratch_bytes(p, L, R, 8, 20, 200)
    want = pair_np(L, R, "left", 5, 0, 32, "sad", (8, 20, 200), 20, True, (1.0, True))
    want2 = sgm_np(L2, R2, "left", 5, 0, 96, "ssd", 8, 40, 200)
    with wslib.WindowSearch(0) as ctx:
        pa = Pair(ctx, L, R)
        t2l, t2r = dev_image(torch, L2), dev_image(torch, R2)
        (l1, r1), (l3, r3) = pa.planes(), pa.planes()
        o2 = torch.full((60, 400), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.search_pair_device(p, pa.tl, pa.tr, l1, r1, (8, 20, 200), 20, 1.0, True, stream=a.cuda_stream)
        ctx.search_sgm_device(p2, t2l, t2r, o2, 8, 40, 200, stream=b.cuda_stream)
        ctx.search_pair_device(p, pa.tl, pa.tr, l3, r3, (8, 20, 200), 20, 1.0, True, stream=a.cuda_stream)
        counts, ucounts = ctx.last_lr_counts(), ctx.last_unique_counts()
        torch.cuda.synchronize()
    for l, r, what in ((l1, r1, "first"), (l3, r3, "again")):
        assert_bits(l.cpu().numpy(), want["checked_left"], what)
        assert_bits(r.cpu().numpy(), want["checked_right"], what)
    assert counts == want["lr_counts"] and ucounts == want["unique_counts"]
    assert_bits(o2.cpu().numpy(), want2, "the SGM call between the two")


def test_cxx_facade_matches_python(wslib, gpu_ctx, tmp_path):
    """tests/cxx/pair_driver.cpp: BlockSearch::computeDisparityMapsCheckedSGM of the C++ facade, both bases."""
    exe = str(tmp_path / "pair_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "pair_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    L, R = shifted_pair(90, 33, 7, 4)
    R = R[:, :85].copy()
    (tmp_path / "l.raw").write_bytes(L.tobytes())
    (tmp_path / "r.raw").write_bytes(R.tobytes())
    outp = tmp_path / "out.raw"
    subprocess.check_call([exe, str(tmp_path / "l.raw"), "90", "33", str(tmp_path / "r.raw"), "85", "33", "5", "1", "24", "40", "300", "8",
                           "1", "1", "20", str(outp)])
    maps = np.frombuffer(outp.read_bytes(), dtype=np.float64)
    nl, nr = 33 * 90, 33 * 85
    assert maps.size == 2 * (nl + nr)
    al, ar = maps[:nl].reshape(33, 90), maps[nl:nl + nr].reshape(33, 85)
    bl, br = maps[nl + nr:2 * nl + nr].reshape(33, 90), maps[2 * nl + nr:].reshape(33, 85)
    want = pair_np(L, R, "left", 5, 1, 24, "ssd", (8, 40, 300), None, False, (1.0, True))
    assert_bits(al, want["checked_left"], "left base, left map")
    assert_bits(ar, want["checked_right"], "left base, right map")
    want = pair_np(L, R, "right", 5, 1, 24, "ssd", (8, 40, 300), 20, False, (1.0, True))
    assert_bits(bl, want["checked_left"], "right base, left map")
    assert_bits(br, want["checked_right"], "right base, right map")
    bs = wslib.BlockSearch(L, R, 5, 1, 24, context=gpu_ctx)
    pl, pr = bs.computeDisparityMapsCheckedSGM(40, 300, 8, 1.0, True)
    assert pl.tobytes() == al.tobytes() and pr.tobytes() == ar.tobytes()
    pl, pr = bs.computeDisparityMapsCheckedSGM(40, 300, 8, 1.0, True, uniquenessRatio=20, base="right")
    assert pl.tobytes() == bl.tobytes() and pr.tobytes() == br.tobytes()
