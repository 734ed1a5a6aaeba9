"""WriteMesh on the device (ws_write_mesh_off_device, ws_reconstruction_host, wsamd::reconstruction): every file must be
byte-identical to the host writer's (ws_write_mesh_off) for the same inputs -- on made-up vertex buffers that reach the
corners of the triangle test and of the %g text, on the reconstruction of real and pipeline maps, and through the C++
facade."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

WS_ERR_ARG, WS_ERR_IO = -1, -5
CALIB = os.path.join(ROOT, "tests", "golden", "teddy_calib.txt")


def _torch():
    import torch
    return torch


def host_text(wslib, tmp_path, pos, col, thr):
    p = str(tmp_path / "host.off")
    wslib.write_mesh_off(p, pos, col, thr)
    with open(p, "rb") as f:
        return f.read()


def device_text(ctx, tmp_path, pos, col, thr, use_torch_stream=False):
    torch = _torch()
    pt = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda()
    ct = torch.from_numpy(np.ascontiguousarray(col, dtype=np.uint8)).cuda()
    p = str(tmp_path / "device.off")
    if use_torch_stream:
        ctx.write_mesh_off_device(pt, ct, thr, p, stream=torch.cuda.current_stream().cuda_stream)
    else:
        torch.cuda.synchronize()
        ctx.write_mesh_off_device(pt, ct, thr, p)
    with open(p, "rb") as f:
        return f.read()


def assert_same(got, want):
    if got == want:
        return
    n = min(len(got), len(want))
    i = next((k for k in range(n) if got[k] != want[k]), n)
    line = want.count(b"\n", 0, i)
    raise AssertionError("texts differ at byte %d (line %d; %d vs %d bytes): device %r host %r" % (
        i, line, len(got), len(want), got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]))


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# the values the %g text must get right: ties, the %f / %e switch, carries, signed zero, the extremes
SPECIAL = np.concatenate([
    np.array([1234565.0, 123456.5, 999999.5, 99999.95, 1e-05, 0.0001, 9.99999e-05, 1e-04, -0.0, 0.0, 1e6, 1e7, 123456.0,
              0.5, -1.5, 3.4028235e38, -3.4028235e38, 1.17549435e-38, 1e-38, 1e30, -1e-30], dtype=np.float32),
    f32([1, 0x80000001, 0x007fffff, 0x00400000, 0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000]),  # subnormals, NaNs, infs
])


def made_up(h, w, seed, thr_hint=1.0):
    """Vertices on a jittered grid (edges within a few ulps of each other) with -inf vertices, NaN / inf coordinates
    and the SPECIAL values sprinkled in."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    pos = np.empty((h, w, 4), dtype=np.float32)
    pos[..., 0] = xs * np.float32(0.1 * thr_hint)
    pos[..., 1] = ys * np.float32(0.1 * thr_hint)
    pos[..., 2] = np.float32(1.0) + rng.standard_normal((h, w)).astype(np.float32) * np.float32(1e-3)
    pos[..., 3] = 1.0
    # a few ulps of jitter on a quarter of the coordinates
    k = rng.integers(-4, 5, size=(h, w, 3)).astype(np.int32)
    k[rng.random((h, w, 3)) < 0.75] = 0
    bits = pos[..., :3].view(np.int32) + k
    pos[..., :3] = bits.view(np.float32)
    flat = pos.reshape(-1, 4)
    n = flat.shape[0]
    pick = rng.random(n)
    flat[pick < 0.08] = -np.inf                                        # invalid vertices (all four -inf)
    sel = (pick >= 0.08) & (pick < 0.11)
    flat[sel, rng.integers(0, 3)] = np.nan                             # NaN coordinates
    sel = (pick >= 0.11) & (pick < 0.13)
    flat[sel, 1] = -np.inf                                             # -inf y: still a valid vertex
    sel = np.nonzero((pick >= 0.13) & (pick < 0.25))[0]
    flat[sel, rng.integers(0, 3, size=sel.size)] = rng.choice(SPECIAL, size=sel.size)
    sel = np.nonzero((pick >= 0.25) & (pick < 0.35))[0]               # big and small magnitudes
    flat[sel, :3] = (rng.standard_normal((sel.size, 3)) * 10.0 ** rng.integers(-40, 38, size=(sel.size, 3))).astype(np.float32)
    col = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    return pos, col


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (41, 1), (2, 2), (3, 257), (5, 300), (17, 1000), (64, 64)])
def test_made_up_vertices_every_shape(wslib, gpu_ctx, tmp_path, shape):
    h, w = shape
    pos, col = made_up(h, w, seed=h * 1000 + w)
    for thr in (1.0, 0.15, float("nan"), float("inf"), -1.0, 0.0):
        assert_same(device_text(gpu_ctx, tmp_path, pos, col, thr), host_text(wslib, tmp_path, pos, col, thr))


def test_edges_within_ulps_of_the_threshold(wslib, gpu_ctx, tmp_path):
    pos, col = made_up(60, 70, seed=5)
    base = float(np.sqrt(np.float32(0.1) * np.float32(0.1) + np.float32(0.1) * np.float32(0.1), dtype=np.float32))
    b = np.array([base], dtype=np.float32).view(np.int32)[0]
    faces = set()
    for ulps in range(-6, 7):
        thr = float(np.array([b + ulps], dtype=np.int32).view(np.float32)[0])
        want = host_text(wslib, tmp_path, pos, col, thr)
        assert_same(device_text(gpu_ctx, tmp_path, pos, col, thr), want)
        faces.add(int(want.split(b"\n")[1].split()[1]))
    assert len(faces) > 3  # the threshold does cut through the triangles here


def test_the_torch_stream_orders_the_call(wslib, gpu_ctx, tmp_path):
    pos, col = made_up(33, 47, seed=9)
    assert_same(device_text(gpu_ctx, tmp_path, pos, col, 1.0, use_torch_stream=True), host_text(wslib, tmp_path, pos, col, 1.0))


def test_a_mesh_over_many_workgroups_and_download_chunks(wslib, gpu_ctx, tmp_path):
    """~900k items (3500 workgroups of 256, four rounds of the scan) and a text of several 8 MB chunks."""
    pos, col = made_up(600, 750, seed=11)
    want = host_text(wslib, tmp_path, pos, col, 1.0)
    assert len(want) > 2 * (8 << 20)
    assert_same(device_text(gpu_ctx, tmp_path, pos, col, 1.0), want)


def reconstruction_pair(wslib, ctx, tmp_path, depth, K, bgr, thr):
    got_p, want_p = str(tmp_path / "rec.off"), str(tmp_path / "two_step.off")
    ctx.reconstruction(depth, K, bgr, thr, got_p)
    pos, col = ctx.back_project(depth, K, bgr)
    wslib.write_mesh_off(want_p, pos, col, thr)
    with open(got_p, "rb") as f:
        got = f.read()
    with open(want_p, "rb") as f:
        want = f.read()
    assert_same(got, want)
    return want


def test_reconstruction_of_teddy_quarter(wslib, gpu_ctx, tmp_path):
    g = load_golden("teddy_quarter")
    K = wslib.read_calib(CALIB)["cam0"]
    disp = wslib.BlockSearch(g["left"], g["right"], 5, 0, 64, cost="sad", context=gpu_ctx).computeDisparityMapLeft(1.0)
    depth = gpu_ctx.convert_disparity_to_depth(disp.astype(np.float32), float(K[0, 0]) / 4, 80.0)
    for thr in (1.0, 50.0, 1e9):
        text = reconstruction_pair(wslib, gpu_ctx, tmp_path, depth, K, g["left"], thr)
    assert int(text.split(b"\n")[1].split()[1]) > 0


def test_reconstruction_of_the_pipeline_chain_at_full_size(wslib, gpu_ctx, tmp_path):
    """main.cpp:40-64 on a 900 x 750 pair: right view 17 x 17, D = 200, smoothFactor 0.9, the 8-bit map, outliers, depth."""
    left, right, _ = make_pair(900, 750, 120, seed=31)
    disp = wslib.BlockSearch(left, right, 17, 0, 200, context=gpu_ctx).computeDisparityMapRight(0.9)
    d8 = np.clip(np.rint(disp), 0, 255).astype(np.float32)
    filt = gpu_ctx.remove_disparity_outliers(d8, 500, 1.5, 0.8)
    depth = gpu_ctx.convert_disparity_to_depth(filt, 3000.0, 1.0)
    K = wslib.read_calib(CALIB)["cam1"]
    text = reconstruction_pair(wslib, gpu_ctx, tmp_path, depth, K, right, 1.0)
    assert text.startswith(b"COFF\n675000 ")


def test_reconstruction_at_1920x1080(wslib, gpu_ctx, tmp_path):
    rng = np.random.default_rng(17)
    h, w = 1080, 1920
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    disp = np.rint(40 + 20 * np.sin(xs / 97.0) * np.cos(ys / 61.0) + rng.integers(-1, 2, size=(h, w))).astype(np.float32)
    disp[rng.random((h, w)) < 0.05] = 0                                      # holes: depth -inf
    depth = gpu_ctx.convert_disparity_to_depth(disp, 3000.0, 0.1)
    bgr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    K = np.array([[3000, 0, 960], [0, 3000, 540], [0, 0, 1]], dtype=np.float32)
    reconstruction_pair(wslib, gpu_ctx, tmp_path, depth, K, bgr, 0.05)


def test_errors(wslib, gpu_ctx, tmp_path):
    torch = _torch()
    lib, h = gpu_ctx._lib, gpu_ctx._h
    pos, col = made_up(4, 5, seed=3)
    pt = torch.from_numpy(pos).cuda()
    ct = torch.from_numpy(col).cuda()
    torch.cuda.synchronize()
    bad = str(tmp_path / "no_such_dir" / "m.off").encode()
    ok = str(tmp_path / "m.off").encode()
    P, C = pt.data_ptr(), ct.data_ptr()
    assert lib.ws_write_mesh_off_device(h, P, C, 5, 4, 1.0, bad, None) == WS_ERR_IO
    assert "cannot open" in lib.ws_last_error(h).decode()
    assert lib.ws_write_mesh_off_device(h, None, C, 5, 4, 1.0, ok, None) == WS_ERR_ARG
    assert lib.ws_write_mesh_off_device(h, P, None, 5, 4, 1.0, ok, None) == WS_ERR_ARG
    assert lib.ws_write_mesh_off_device(h, P, C, 5, 4, 1.0, None, None) == WS_ERR_ARG
    assert lib.ws_write_mesh_off_device(None, P, C, 5, 4, 1.0, ok, None) == WS_ERR_ARG
    for w_, h_ in ((0, 4), (5, 0), (-1, 4), (5, -3), (70000, 70000), (65536, 65537)):
        assert lib.ws_write_mesh_off_device(h, P, C, w_, h_, 1.0, ok, None) == WS_ERR_ARG, (w_, h_)
    assert "32-bit" in lib.ws_last_error(h).decode()
    assert lib.ws_write_mesh_off_device(h, P + 4, C, 5, 4, 1.0, ok, None) == WS_ERR_ARG  # misaligned positions
    assert not os.path.exists(ok)                                                       # nothing was opened
    if os.path.exists("/dev/full"):                                                     # a write that fails
        assert lib.ws_write_mesh_off_device(h, P, C, 5, 4, 1.0, b"/dev/full", None) == WS_ERR_IO
        big_p, big_c = made_up(600, 750, seed=2)
        with pytest.raises(wslib.WsError) as e:
            gpu_ctx.write_mesh_off_device(torch.from_numpy(big_p).cuda(), torch.from_numpy(big_c).cuda(), 1.0, "/dev/full",
                                          stream=torch.cuda.current_stream().cuda_stream)
        assert e.value.code == WS_ERR_IO
    # the call still works after the failures
    assert_same(device_text(gpu_ctx, tmp_path, pos, col, 1.0), host_text(wslib, tmp_path, pos, col, 1.0))

    depth = np.full((4, 5), 2.0, dtype=np.float32)
    bgr = np.zeros((4, 5, 3), dtype=np.uint8)
    K = np.eye(3, dtype=np.float32)
    with pytest.raises(wslib.WsError) as e:
        gpu_ctx.reconstruction(depth, K, bgr, 1.0, bad.decode())
    assert e.value.code == WS_ERR_IO
    with pytest.raises(wslib.WsError) as e:
        gpu_ctx.reconstruction(depth, K, np.zeros((4, 6, 3), dtype=np.uint8), 1.0, ok.decode())
    assert e.value.code == WS_ERR_ARG
    k9 = (ctypes.c_float * 9)(*K.reshape(9))
    img = wslib._Image(bgr.ctypes.data, 5, 4, 15)
    assert lib.ws_reconstruction_host(h, None, 5, 4, 5, k9, ctypes.byref(img), 1.0, ok) == WS_ERR_ARG
    assert lib.ws_reconstruction_host(h, depth.ctypes.data, 5, 4, 4, k9, ctypes.byref(img), 1.0, ok) == WS_ERR_ARG
    assert lib.ws_reconstruction_host(h, depth.ctypes.data, 5, 4, 5, None, ctypes.byref(img), 1.0, ok) == WS_ERR_ARG
    assert lib.ws_reconstruction_host(h, depth.ctypes.data, 5, 4, 5, k9, None, 1.0, ok) == WS_ERR_ARG
    assert not os.path.exists(ok)
    assert lib.ws_reconstruction_host(h, depth.ctypes.data, 5, 4, 5, k9, ctypes.byref(img), 1.0, ok) == 0
    assert open(ok, "rb").read().startswith(b"COFF\n20 ")


def test_cxx_facade_reconstruction_equals_the_host_writer(wslib, tmp_path):
    exe = str(tmp_path / "mesh_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "mesh_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    rng = np.random.default_rng(23)
    h, w = 140, 240
    disp = rng.integers(0, 60, size=(h, w)).astype(np.float32)
    depth = np.where(disp == 0, -np.inf, np.float32(3000.0) / np.maximum(disp, 1)).astype(np.float32)
    bgr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    dp, bp = str(tmp_path / "depth.raw"), str(tmp_path / "bgr.raw")
    depth.tofile(dp)
    bgr.tofile(bp)
    fa, ho = str(tmp_path / "facade.off"), str(tmp_path / "host.off")
    for thr in ("1.0", "40", "1e9"):
        subprocess.check_call([exe, dp, bp, str(w), str(h), "3000", "120", "3000", "70", thr, fa, ho])
        assert_same(open(fa, "rb").read(), open(ho, "rb").read())
    # an unwritable path: the reference's message, the status in the exit code (10 - WS_ERR_IO)
    r = subprocess.run([exe, dp, bp, str(w), str(h), "3000", "120", "3000", "70", "1.0", str(tmp_path / "nope" / "m.off"), ho],
                       capture_output=True, text=True)
    assert r.returncode == 15 and "Failed to write mesh! Check file path!" in r.stdout
