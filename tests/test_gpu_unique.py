"""The uniqueness ratio and confidence calls on the device (ws_search_unique_device / _host, ws_last_unique_counts,
BlockSearch::computeDisparityMapLeftUnique / RightUnique): whole maps and confidence planes as float32 bits, and the
counts, against tests/unique_ref.py -- on the staircases of tests/unique_inputs.py (every stored type of the winner
kernel), at the smallest disparity ranges and around 64, on census costs, on images of unequal sizes, with sub-pixel, on
padded planes, through the host form, across streams that share the scratch, and through the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sgm_inputs import geometry_case
from test_gpu_sgm import assert_bits, dev_image, params_of
from test_subpixel_reference import shifted_pair
from unique_inputs import RATIOS, STAIRCASES, VARIANTS, case, reference, sgm_of
from unique_ref import sums, unique_from_sums, volume

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


class Pair:
    """A pair on the device, and uniqueness calls on it into fresh NaN-filled planes."""

    def __init__(self, wslib, ctx, L, R, view, pad=0):
        torch = _torch()
        self.wslib, self.ctx, self.view, self.pad = wslib, ctx, view, pad
        self.tl, self.tr = dev_image(torch, L, pad), dev_image(torch, R, pad)
        self.h, self.w = (L if view == "left" else R).shape[:2]

    def plane(self, pad):
        return _torch().full((self.h, self.w + pad), float("nan"), dtype=_torch().float32, device="cuda")

    def run(self, params, ratio, sgm, conf=True, stream=None):
        """(map, confidence or None, counts)"""
        torch = _torch()
        out, cf = self.plane(self.pad), self.plane(2 * self.pad) if conf else None
        s = stream.cuda_stream if stream is not None else None
        self.ctx.search_unique_device(params, self.tl, self.tr, out[:, :self.w], ratio, sgm,
                                      None if cf is None else cf[:, :self.w], stream=s)
        counts = self.ctx.last_unique_counts()
        torch.cuda.synchronize()
        res = []
        for t in (out, cf):
            if t is None:
                res.append(None)
                continue
            a = t.cpu().numpy()
            assert np.isnan(a[:, self.w:]).all(), "the padding of the rows was written"
            res.append(a[:, :self.w])
        return res[0], res[1], counts


def check(pair, params, ratio, sgm, want, what):
    got, conf, counts = pair.run(params, ratio, sgm)
    assert_bits(got, want["map"], ("map",) + what)
    assert_bits(conf, want["conf"], ("conf",) + what)
    assert counts == want["counts"], (what, counts, want["counts"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", STAIRCASES)
def test_staircases(wslib, gpu_ctx, name, variant):
    L, R, (view, bs, mind, maxd, cost), _, nd, V = case(name)
    pair = Pair(wslib, gpu_ctx, L, R, view, pad=3 if variant == "zero" else 0)
    sub = variant == "sgm"
    p = params_of(wslib, view, bs, mind, maxd, cost, sub)
    for ratio in RATIOS:
        check(pair, p, ratio, sgm_of(name, variant), reference(name, variant, ratio, subpixel=sub), (name, variant, ratio))


def reference_of(L, R, view, bs, mind, maxd, cost, ratio, sgm, sub):
    V = volume(L, R, view, bs, mind, maxd, cost)
    return V, unique_from_sums(V, sums(V, sgm), view, ratio, sub)


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("nd", [1, 2, 3, 4, 5, 63, 64, 65, 66])
def test_small_ranges(wslib, gpu_ctx, nd, view):
    """nd <= 2: every node is uncontested; nd = 3: only a winner at an end has a rival; nd = 4: rivals at distance 2 or 3;
    63 .. 66: the last lane of the first row, and the first lanes of the second."""
    w, h = (24, 10) if nd <= 5 else (100, 6)
    mind = 2 if view == "right" and nd % 2 else 0
    L, R = shifted_pair(w, h, max(1, min(nd // 2, 9)), 300 + nd)
    pair = Pair(wslib, gpu_ctx, L, R, view)
    p = params_of(wslib, view, 3, mind, mind + nd if view == "right" else nd, "sad", nd % 2 == 0)
    seen = 0
    for sgm in ((8, 5, 40), None):
        for ratio in (15, 100):
            V, want = reference_of(L, R, view, 3, mind, p.max_disparity, "sad", ratio, sgm, nd % 2 == 0)
            assert V[0].shape[0] == nd
            check(pair, p, ratio, sgm, want, (nd, view, sgm, ratio))
            count = (V[0] >= 0).sum(axis=0)
            assert not (want["contested"] & (count <= 2)).any()
            if nd <= 2:
                assert not want["contested"].any() and want["counts"][0] == 0 and want["counts"][1] > 0
            seen += int(want["contested"].sum())
    assert (seen > 0) == (nd >= 3)


@pytest.mark.parametrize("cost,bs", [("census5x5", 5), ("census9x7", 7)])
def test_census(wslib, gpu_ctx, cost, bs):
    L, R = shifted_pair(97, 23, 11, 41)
    for view, mind in (("left", 0), ("right", 1)):
        pair = Pair(wslib, gpu_ctx, L, R, view)
        p = params_of(wslib, view, bs, mind, 70, cost, True)
        for sgm in (None, (8, 3, 20)):
            V, want = reference_of(L, R, view, bs, mind, 70, cost, 15, sgm, True)
            assert want["counts"][0] > 5 and int((want["contested"] & ~want["fail"]).sum()) > 5
            check(pair, p, 15, sgm, want, (cost, view, sgm))


@pytest.mark.parametrize("name", ["right-wider-min", "left-wider-taller"])
def test_geometry(wslib, gpu_ctx, name):
    """Columns without a candidate (-x, confidence 0) and rows outside the searched region (0, confidence 0)."""
    maxd = 12
    L, R, view, mind = geometry_case(name, 61, 17, maxd)
    pair = Pair(wslib, gpu_ctx, L, R, view, pad=2)
    p = params_of(wslib, view, 5, mind, maxd, "ssd", True)
    for sgm in (None, (4, 60, 900)):
        V, want = reference_of(L, R, view, 5, mind, maxd, "ssd", 20, sgm, True)
        node = V[2]
        assert (~node).sum() > 50 and (want["conf"][~node] == 0).all()
        if view == "right":
            assert (want["map"][:, L.shape[1]:] < 0).any()
        check(pair, p, 20, sgm, want, (name, sgm))


@pytest.mark.parametrize("view", ["left", "right"])
def test_subpixel_with_a_ratio(wslib, gpu_ctx, view):
    L, R = shifted_pair(140, 37, 13, 7)
    pair = Pair(wslib, gpu_ctx, L, R, view)
    p = params_of(wslib, view, 5, 1 if view == "right" else 0, 40, "ssd", True)
    for sgm in (None, (8, 300, 3000)):
        V, want = reference_of(L, R, view, 5, p.min_disparity, 40, "ssd", 30, sgm, True)
        kept = V[2] & ~want["fail"]
        assert (want["map"][kept] != np.round(want["map"][kept])).sum() > 100, "refined values among the kept nodes"
        assert want["counts"][0] > 20
        check(pair, p, 30, sgm, want, (view, sgm))


def test_device_identities(wslib, gpu_ctx):
    """Ratio 0 is ws_search_sgm_device's map, without sgm ws_search_device's; sgm == NULL equals {8, 0, 0} at any ratio."""
    torch = _torch()
    L, R = shifted_pair(300, 61, 21, 12)
    for view, sub in (("left", True), ("right", False), ("right", True)):
        pair = Pair(wslib, gpu_ctx, L, R, view)
        p = params_of(wslib, view, 7, 0, 96, "ssd", sub)
        want = pair.plane(0)
        gpu_ctx.search_sgm_device(p, pair.tl, pair.tr, want, 8, 200, 1800)
        torch.cuda.synchronize()
        got, _, counts = pair.run(p, 0, (8, 200, 1800))
        assert_bits(got, want.cpu().numpy(), ("sgm", view, sub))
        assert counts[0] == 0 and counts[1] > 0
        block = pair.plane(0)
        gpu_ctx.search_device(p, pair.tl, pair.tr, block)
        torch.cuda.synchronize()
        got, _, _ = pair.run(p, 0, None)
        assert_bits(got, block.cpu().numpy(), ("block", view, sub))
        for ratio in (15, 100):
            a, ca, na = pair.run(p, ratio, None)
            b, cb, nb = pair.run(p, ratio, (8, 0, 0))
            assert_bits(a, b, ("none / zero", view, ratio))
            assert_bits(ca, cb, ("none / zero, confidence", view, ratio))
            assert na == nb and na[0] > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planes_strides_and_the_host_form(wslib, gpu_ctx, dtype):
    L, R = shifted_pair(150, 47, 9, 3)
    L = L.copy()
    L[20:24, 30:70] = 0
    for view, sgm in (("left", (8, 300, 3000)), ("right", None)):
        p = params_of(wslib, view, 5, 0, 48, "ssd", True)
        pair = Pair(wslib, gpu_ctx, L, R, view, pad=7)   # (Pair.run checks the padding of both planes)
        want, conf, counts = pair.run(p, 25, sgm)
        alone, none, counts2 = pair.run(p, 25, sgm, conf=False)
        assert none is None and counts2 == counts
        assert_bits(alone, want, (view, "without a confidence plane"))
        got, gconf = gpu_ctx.search_unique(p, L, R, 25, sgm, dtype=dtype, conf=True)
        assert got.dtype == dtype and gconf.dtype == np.float32
        assert gpu_ctx.last_host_paths() == ("staged",) * 3
        assert gpu_ctx.last_unique_counts() == counts
        assert_bits(got.astype(np.float32), want, (view, "host map"))
        assert got.astype(np.float32).astype(dtype).tobytes() == got.tobytes()
        assert_bits(gconf, conf, (view, "host confidence"))
        only = gpu_ctx.search_unique(p, L, R, 25, sgm, dtype=dtype)
        assert only.tobytes() == got.tobytes()


def test_shared_scratch_across_streams(wslib):
    """A uniqueness call on stream A, an SGM call that needs more scratch on stream B, the first again, on a context of
    their own (its scratch starts empty): the scratch is one buffer, grown in between, and the calls order themselves."""
    torch = _torch()
    from sgm_ref import sgm_np
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    L, R = shifted_pair(120, 40, 9, 9)
    L2, R2 = shifted_pair(400, 60, 30, 10)
    p = params_of(wslib, "left", 5, 0, 32, "sad", True)
    p2 = params_of(wslib, "left", 5, 0, 96, "ssd")
    assert wslib.sgm_scratch_bytes(p2, L2, R2, 8, 40, 200) > 4 * wslib.unique_scratch_bytes(p, L, R, None)
    _, want = reference_of(L, R, "left", 5, 0, 32, "sad", 20, None, True)
    want2 = sgm_np(L2, R2, "left", 5, 0, 96, "ssd", 8, 40, 200)
    with wslib.WindowSearch(0) as ctx:
        pa = Pair(wslib, ctx, L, R, "left")
        t2l, t2r = dev_image(torch, L2), dev_image(torch, R2)
        o1, c1, o3, c3 = pa.plane(0), pa.plane(0), pa.plane(0), pa.plane(0)
        o2 = torch.full((60, 400), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.search_unique_device(p, pa.tl, pa.tr, o1, 20, None, c1, stream=a.cuda_stream)
        ctx.search_sgm_device(p2, t2l, t2r, o2, 8, 40, 200, stream=b.cuda_stream)
        ctx.search_unique_device(p, pa.tl, pa.tr, o3, 20, None, c3, stream=a.cuda_stream)
        counts = ctx.last_unique_counts()
        torch.cuda.synchronize()
    for o, c, what in ((o1, c1, "first"), (o3, c3, "again")):
        assert_bits(o.cpu().numpy(), want["map"], what)
        assert_bits(c.cpu().numpy(), want["conf"], what)
    assert counts == want["counts"]
    assert_bits(o2.cpu().numpy(), want2, "the SGM call between the two")


def test_cxx_facade_matches_python(wslib, gpu_ctx, tmp_path):
    """tests/cxx/unique_driver.cpp: BlockSearch::computeDisparityMapLeftUnique / RightUnique of the C++ facade."""
    exe = str(tmp_path / "unique_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "unique_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    L, R = shifted_pair(90, 33, 7, 4)
    R = R[:, :85].copy()
    (tmp_path / "l.raw").write_bytes(L.tobytes())
    (tmp_path / "r.raw").write_bytes(R.tobytes())
    outp = tmp_path / "out.raw"
    subprocess.check_call([exe, str(tmp_path / "l.raw"), "90", "33", str(tmp_path / "r.raw"), "85", "33", "5", "1", "24", "20", "40",
                           "300", "8", str(outp)])
    raw = outp.read_bytes()
    nl, nr = 33 * 90, 33 * 85
    maps = np.frombuffer(raw[:8 * (2 * nl + nr)], dtype=np.float64)
    confs = np.frombuffer(raw[8 * (2 * nl + nr):], dtype=np.float32)
    assert confs.size == nl + nr
    block, left, right = maps[:nl].reshape(33, 90), maps[nl:2 * nl].reshape(33, 90), maps[2 * nl:].reshape(33, 85)
    cblock, cright = confs[:nl].reshape(33, 90), confs[nl:].reshape(33, 85)
    for what, got, conf, view, mind, sgm in (("block", block, cblock, "left", 0, None), ("left", left, None, "left", 0, (8, 40, 300)),
                                             ("right", right, cright, "right", 1, (8, 40, 300))):
        _, want = reference_of(L, R, view, 5, mind, 24, "ssd", 20, sgm, False)
        assert_bits(got, want["map"], what)
        if conf is not None:
            assert_bits(conf, want["conf"], what)
        p = params_of(wslib, view, 5, mind, 24, "ssd")
        assert got.tobytes() == gpu_ctx.search_unique(p, L, R, 20, sgm, dtype=np.float64).tobytes(), what
