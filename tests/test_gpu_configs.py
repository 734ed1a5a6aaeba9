"""BASELINE.json configs that round 1 left without a device test: config 4 (the 15 trainingH shapes,
batched and device-resident), config 5 WITH the sub-pixel refine at D = 1024 (four d-group passes
meeting in the key plane before the parabola), and a MotorcycleE-shaped unequal pair at full size
(results/Rectified/trainingH/MotorcycleE: 1481 x 1038 left, 1495 x 1052 right, SURVEY.md section 2
row 15).  Full maps are checked through size-independent properties, oracle row bands bit for bit.
"""
import ctypes

import numpy as np
import pytest

from stereo_reconstruction_amd.synthetic import TRAINING_H, make_pair


pytestmark = pytest.mark.gpu

SUBPIXEL_TOL = 1e-4     # north_star: "within 1e-4 for float"


def left_view_properties(got, gt, bs, maxd, w2=None):
    """What holds for every left-view map of a synthetic pair (BlockSearch.cpp:24-86), any size."""
    h, w = got.shape
    half = (bs - 1) // 2
    assert (got[:half] == 0).all() and (got[h - half:] == 0).all()
    assert (got[:, :half] == 0).all() and (got[:, w - half:] == 0).all()
    assert (got[half:h - half, half] == half).all()             # x = half: no candidate -> stores x
    inner = got[half:h - half, half:w - half]
    assert inner.min() >= 1 and inner.max() <= max(maxd, w) and (inner == np.round(inner)).all()
    x_hi = w - half if w2 is None else min(w - half, w2 - half)
    hit = (got[half:h - half, maxd:x_hi] == gt[half:h - half, maxd:x_hi]).mean() if x_hi > maxd else 1.0
    assert hit > 0.6, hit


def bands(h, half, n):
    return [(half, half + n), (h // 2, h // 2 + n), (h - half - n, h - half)]


@pytest.mark.parametrize("view", ["left", "right"])
def test_config3_full_size_sad_with_the_halo_exchange(wslib, gpu_ctx, oracle, view):
    """BASELINE.json configs[2] at full size (2964 x 1988, 9x9 SAD, D = 512): the packed SAD kernel whose threads take
    the right-hand part of their windows from the neighbouring thread -- tiles of 16 runs overlapping by one, 16 disparities
    per thread: the 512 candidates in one pass -- against oracle row bands over the full width (every tile seam)."""
    import torch
    w, h, bs, maxd = 2964, 1988, 9, 512
    half = (bs - 1) // 2
    left, right, gt = make_pair(w, h, maxd, 33)
    p = wslib.make_params(wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT, bs, 0, maxd, 1.0, "sad")
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    to = torch.empty((h, w), dtype=torch.float32, device="cuda")
    gpu_ctx.search_device(p, tl, tr, to, None)
    torch.cuda.synchronize()
    info = gpu_ctx.last_launch()
    assert "halo" in info["kernel"] and info["threads"] == 512, info
    got = to.cpu().numpy().astype(np.float64)
    fn = oracle.block_left if view == "left" else oracle.block_right
    for y0, y1 in bands(h, half, 2):
        band = fn(left, right, bs, 0, maxd, cost="sad", rows=(y0, y1), threads=8)
        assert np.array_equal(got[y0:y1], band[y0:y1]), (view, y0)
    if view == "left":
        left_view_properties(got, gt, bs, maxd)


@pytest.mark.parametrize("dmode", ["D256", "ndisp"])
def test_config4_training_h_shapes(wslib, gpu_ctx, oracle, dmode):
    """BASELINE.json configs[3]: 15 pairs with the trainingH shapes, 7x7 SSD, D = 256 and D = ndisp
    (each scene's calib.txt), through the batched host entry points (ws_enqueue_host ... ws_wait) and
    through ws_search_device; both must give the same bits, three oracle row bands per pair."""
    import torch
    bs = 7
    half = 3
    pairs, ds = [], []
    for i, (_name, w, h, ndisp) in enumerate(TRAINING_H):
        maxd = 256 if dmode == "D256" else ndisp
        pairs.append(make_pair(w, h, maxd, 100 + i))
        ds.append(maxd)
    if dmode == "D256":
        p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, 256, 1.0, "ssd")
        many = gpu_ctx.search_many(p, [(l, r) for l, r, _ in pairs], dtype=np.float32)
    else:   # the range is a parameter of the call: one enqueue per pair with its own D, one wait
        import ctypes
        lib = wslib.load_library()
        keep, many = [], []
        for (l, r, _), maxd in zip(pairs, ds):
            p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, maxd, 1.0, "ssd")
            La, Li = wslib._host_image(l)
            Ra, Ri = wslib._host_image(r)
            out = np.empty(La.shape[:2], dtype=np.float32)
            assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri),
                                       out.ctypes.data, out.shape[1], 0) == 0
            keep.append((La, Ra, p))
            many.append(out)
        assert lib.ws_wait(gpu_ctx._h) == 0
    for i, ((l, r, gt), maxd, got) in enumerate(zip(pairs, ds, many)):
        name, w, h, _ = TRAINING_H[i]
        assert got.shape == (h, w)
        p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, maxd, 1.0, "ssd")
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        to = torch.empty((h, w), dtype=torch.float32, device="cuda")
        gpu_ctx.search_device(p, tl, tr, to, None)
        torch.cuda.synchronize()
        assert "march" in gpu_ctx.last_launch()["kernel"], name
        assert np.array_equal(to.cpu().numpy(), got), name
        g64 = got.astype(np.float64)
        for y0, y1 in bands(h, half, 2):
            band = oracle.block_left(l, r, bs, 0, maxd, cost="ssd", rows=(y0, y1), threads=8)
            assert np.array_equal(g64[y0:y1], band[y0:y1]), (name, maxd, y0)
        left_view_properties(g64, gt, bs, maxd)


def test_config5_subpixel_at_full_size(wslib, gpu_ctx, oracle):
    """BASELINE.json configs[4]: 3840 x 2160, 9x9 SSD, D = 1024, parabolic refine.  D = 1024 runs as four
    d-group passes whose keys meet in a plane (ws_march.hip) BEFORE the refine reads the winner: the
    integer part must be the bit-exact argmin (BlockSearch.cpp:76-82), the fraction within 1e-4 of the double
    refinement and the float32 value exactly the one the device's arithmetic defines."""
    w, h, bs, maxd = 3840, 2160, 9, 1024
    half = 4
    left, right, gt = make_pair(w, h, maxd, 5)
    p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, maxd, 1.0, "ssd")
    assert wslib.plan(p, left.shape, right.shape)["passes"] == 4
    whole = wslib.BlockSearch(left, right, bs, 0, maxd, cost="ssd", context=gpu_ctx).computeDisparityMapLeft(1.0)
    sub = wslib.BlockSearch(left, right, bs, 0, maxd, cost="ssd", subpixel=True, context=gpu_ctx).computeDisparityMapLeft(1.0)
    assert "march" in gpu_ctx.last_launch()["kernel"]
    left_view_properties(whole, gt, bs, maxd)
    # the refine moves a disparity by at most half a step and never touches border / fallback pixels
    frac = sub - whole
    assert np.abs(frac).max() <= 0.5 + SUBPIXEL_TOL
    assert (frac[:half] == 0).all() and (frac[:, :half] == 0).all() and (frac[half:h - half, half] == 0).all()
    assert (frac != 0).mean() > 0.5         # and it does move most pixels
    for y0, y1 in bands(h, half, 2):
        want_int = oracle.block_left(left, right, bs, 0, maxd, cost="ssd", rows=(y0, y1), threads=8)
        want_sub = oracle.block_left(left, right, bs, 0, maxd, cost="ssd", subpixel=True, rows=(y0, y1), threads=8)
        assert np.array_equal(whole[y0:y1], want_int[y0:y1]), y0
        err = np.abs(sub[y0:y1] - want_sub[y0:y1]).max()
        assert err <= SUBPIXEL_TOL, (y0, err)
        want_f32 = oracle.block_left(left, right, bs, 0, maxd, cost="ssd", subpixel="float32", rows=(y0, y1), threads=8)
        assert np.array_equal(sub[y0:y1], want_f32[y0:y1]), (y0, np.argwhere(sub[y0:y1] != want_f32[y0:y1])[:5].tolist())
        # integer part of the refined map == the argmin, recovered without the oracle's own fraction
        assert np.array_equal(np.round(sub[y0:y1] - (want_sub[y0:y1] - want_int[y0:y1])), want_int[y0:y1]), y0


def test_motorcycle_e_shaped_unequal_pair(wslib, gpu_ctx, oracle):
    """Left 1481 x 1038, right 1495 x 1052 (the rectified MotorcycleE pair's shapes) with ~5 % black
    border as the rectifying warp leaves it.  Left view in both orders; the right view is only legal
    when the left image is at least as tall (BlockSearch.cpp:151-154 throws otherwise)."""
    w1, h1, w2, h2, maxd = 1481, 1038, 1495, 1052, 140
    left, right, gt = make_pair(w1, h1, maxd, 31, right_width=w2, right_height=h2)
    left[:, :30] = 0
    left[:12] = 0
    right[:, w2 - 40:] = 0
    right[h2 - 20:] = 0
    half = 3
    got = wslib.BlockSearch(left, right, 7, 0, maxd, cost="ssd", context=gpu_ctx).computeDisparityMapLeft(1.0)
    assert "march" in gpu_ctx.last_launch()["kernel"]
    assert got.shape == (h1, w1)
    for y0, y1 in bands(h1, half, 2) + [(12, 14)]:
        band = oracle.block_left(left, right, 7, 0, maxd, cost="ssd", rows=(y0, y1), threads=8)
        assert np.array_equal(got[y0:y1], band[y0:y1]), y0
    assert (got[:12] == 0).all() and (got[:, :30] == 0).all()      # black pixels are skipped
    # the right view of this pair: the reference throws (left image too short for the bottom windows)
    with pytest.raises(wslib.WsError) as e:
        wslib.BlockSearch(left, right, 7, 0, maxd, context=gpu_ctx).computeDisparityMapRight(1.0)
    assert e.value.code == -2
    # swapped roles: taller / wider image on the left -> both views legal, map sizes differ
    b = wslib.BlockSearch(right, left, 7, 0, maxd, cost="sad", context=gpu_ctx)
    gl = b.computeDisparityMapLeft(1.0)
    gr = b.computeDisparityMapRight(1.0)
    assert gl.shape == (h2, w2) and gr.shape == (h1, w1)
    assert (gl[h1 - half:] == 0).all()                              # rows >= min(h1,h2) - half stay 0
    for y0, y1 in bands(h1, half, 2):
        assert np.array_equal(gl[y0:y1], oracle.block_left(right, left, 7, 0, maxd, cost="sad", rows=(y0, y1), threads=8)[y0:y1])
    for y0, y1 in [(0, 2), (h1 // 2, h1 // 2 + 2), (h1 - 2, h1)]:
        assert np.array_equal(gr[y0:y1], oracle.block_right(right, left, 7, 0, maxd, cost="sad", rows=(y0, y1), threads=8)[y0:y1])


@pytest.mark.parametrize("cfg", [("config2", 1500, 1000, 7, "ssd", 256, 2), ("config3", 2964, 1988, 9, "sad", 512, 3),
                                 ("config5", 3840, 2160, 9, "ssd", 1024, 5)])
def test_the_planners_plan_is_within_5_percent_of_the_best_forced_one(wslib, cfg):
    """The tiling plan is a pile of constants fitted on one box (march_plan: strip model, 256- vs 512-thread workgroups,
    halo-exchange tiles).  This replaces the by-hand check of round 3 (profiles/r03/nd_rule_check.txt): the automatic
    plan against the forced alternatives ws_set_tuning can ask for -- workgroup size 256 / 512 x tile widths 4 / 8 / 16
    x-runs (8 and 16: the halo-exchange kernels where they exist) -- device-resident, best of three timings each.
    All plans must give the SAME map."""
    import torch
    name, w, h, bs, cost, maxd, seed = cfg
    left, right, _ = make_pair(w, h, maxd, seed)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, maxd, 1.0, cost)
    st = torch.cuda.current_stream().cuda_stream
    reps = 8 if name == "config2" else 3

    def timed(ctx):
        for _ in range(2):
            ctx.search_device(p, tl, tr, out, st)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            ctx.timer_begin(st)
            for _ in range(reps):
                ctx.search_device(p, tl, tr, out, st)
            best = min(best, ctx.timer_end(st) / reps)
        return best, out.clone()

    with wslib.WindowSearch(0) as ctx:
        timed(ctx)                                # (clocks up, code loaded: the first timing of a process runs 5-8 % long)
        auto_ms, auto_map = timed(ctx)
        auto_plan = ctx.last_launch()
        results = {}
        for threads in (256, 512):
            for nxr in (0, 4, 8, 16):
                try:
                    ctx.set_tuning(nxr, 0, threads)
                    ms, m = timed(ctx)
                except wslib.WsError:
                    continue                      # (a tuning the planner cannot satisfy)
                assert torch.equal(m, auto_map), (name, threads, nxr)
                results[(threads, nxr)] = (ms, ctx.last_launch()["kernel"])
        ctx.set_tuning(0, 0, 0)
        auto_ms = min(auto_ms, timed(ctx)[0])     # (and once more after the others: the box's drift is not the planner's)
    best_key = min(results, key=lambda k: results[k][0])
    best_ms = results[best_key][0]
    print("%s: auto %.4f ms (%s, %d threads); best forced %.4f ms %s %s" % (name, auto_ms, auto_plan["kernel"], auto_plan["threads"],
                                                                            best_ms, best_key, results[best_key][1]))
    assert auto_ms <= 1.05 * best_ms, (name, auto_ms, auto_plan, {k: round(v[0], 4) for k, v in results.items()})


@pytest.mark.parametrize("view", ["left", "right"])
def test_device_images_at_any_byte_alignment_and_stride(wslib, oracle, view):
    """The marching kernel reads the caller's CV_8UC3 bytes itself (round 4): 16-byte blocks by LDS-DMA from wherever
    a row starts, unpacked with the row's own byte phase.  Device-resident images cut out of a byte buffer at every
    phase of 16, with row strides that are odd, a multiple of 4 but not 16, and a multiple of 16 -- cv::Mat ROIs and
    tightly packed rows of any width -- SSD and SAD, the plain and the halo-exchange kernels, both views; the buffers
    around the images are poisoned (a kernel that reads a neighbour's bytes as its own shows)."""
    import torch
    rng = np.random.default_rng(17)
    w, h, bs = 333, 40, 7
    left, right, _ = make_pair(w, h, 48, seed=71)
    left[20, 100] = 0
    right[21, 90] = 0
    for cost, maxd in (("ssd", 48), ("sad", 300)):
        want = (oracle.block_left if view == "left" else oracle.block_right)(left, right, bs, 0, maxd, cost=cost, threads=8)
        p = wslib.make_params(wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT, bs, 0, maxd, 1.0, cost)
        with wslib.WindowSearch(0) as ctx:
            for off, stride in ((0, 3 * w), (1, 3 * w), (2, 3 * w + 1), (3, 3 * w + 5), (5, 1004), (7, 1008), (11, 1024), (13, 3 * w + 2), (15, 1040)):
                bufs = []
                for img in (left, right):
                    raw = torch.from_numpy(rng.integers(0, 256, size=off + stride * h + 64, dtype=np.uint8)).cuda()
                    view2d = raw[off:off + stride * h].view(h, stride)
                    view2d[:, :3 * w] = torch.from_numpy(img.reshape(h, 3 * w)).cuda()
                    bufs.append((raw, raw.data_ptr() + off, stride))
                out = torch.full((h, w), -3.0, dtype=torch.float32, device="cuda")
                Li = wslib._Image(bufs[0][1], w, h, bufs[0][2])
                Ri = wslib._Image(bufs[1][1], w, h, bufs[1][2])
                lib = wslib.load_library()
                rc = lib.ws_search_device(ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), out.data_ptr(), w, None)
                assert rc == 0, lib.ws_last_error(ctx._h)
                torch.cuda.synchronize()
                assert "march" in ctx.last_launch()["kernel"]
                assert np.array_equal(out.cpu().numpy().astype(np.float64), want), (view, cost, off, stride)
