"""Whole disparity maps, every pixel, against the fast exact CPU reference (oracle.fast_left / fast_right,
oracle/ws_fast.c, pinned to the line-cited oracle by tests/test_fast_reference.py).

The older full-size tests compare a few row bands with the oracle, which needs minutes per full-size view; a tile
seam or strip boundary between the sampled rows would pass them.  Here:
  * the BASELINE.json configs at full size (bench.WORKLOADS shapes and seeds), both views, sub-pixel at config 5,
    config 4's 15 trainingH shapes, the MotorcycleE-shaped unequal pair, the reference's pipeline call and the
    left view's raster bands with smoothFactor != 1;
  * a seam sweep whose shapes come from the planner (ws_plan) at test time: the image edge at the last strip's
    first and second-to-last row, the last tile's first and second-to-last column, D at a whole number of d-chunks
    and one either side, both sides of every change of the d-group pass count (one pass to several,
    3 -> 4), D clamped by the width -- each case
    asserts the plan has the seam it names and the kernel it names ran;
  * key-range extremes: windows whose every candidate costs the analytic maximum (only the tie tag decides), one
    candidate one unit below it, D at the last value the marching kernel accepts and the first it refuses, a
    multi-pass D, the smooth path's top-3 table and the brute-force kernel at the largest window (63).
Integer maps are compared with np.array_equal; sub-pixel maps within 1e-4 of the double refinement and with
np.array_equal against the float32 value the device's arithmetic defines (tests/test_gpu_subpixel.py).
"""
import numpy as np
import pytest

from stereo_reconstruction_amd.synthetic import TRAINING_H, make_pair

pytestmark = pytest.mark.gpu

SUBPIXEL_TOL = 1e-4
WORKLOADS = {    # bench.WORKLOADS: (width, height, block, cost, maxD, seed)
    "config1": (450, 375, 5, "sad", 64, 1),
    "config2": (1500, 1000, 7, "ssd", 256, 2),
    "config3": (2964, 1988, 9, "sad", 512, 3),
    "config5": (3840, 2160, 9, "ssd", 1024, 5),
}


def _view(wslib, view):
    return wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT


def _fast(oracle, view):
    return oracle.fast_left if view == "left" else oracle.fast_right


def _search(wslib, ctx, view, left, right, bs, mind, maxd, cost, smooth=1.0, subpixel=False):
    p = wslib.make_params(_view(wslib, view), bs, mind, maxd, smooth, cost, subpixel=subpixel)
    return ctx.search(p, left, right)


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s)"
                             % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- 1. BASELINE configs, whole maps -------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("name", ["config1", "config2", "config5"])
def test_config_whole_map(wslib, gpu_ctx, oracle, name, view):
    w, h, bs, cost, maxd, seed = WORKLOADS[name]
    left, right, _ = make_pair(w, h, maxd, seed)
    got = _search(wslib, gpu_ctx, view, left, right, bs, 0, maxd, cost)
    assert "march" in gpu_ctx.last_launch()["kernel"], gpu_ctx.last_launch()
    _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost=cost), (name, view))


@pytest.mark.parametrize("view", ["left", "right"])
def test_config3_whole_map_through_the_halo_packed_sad_kernel(wslib, gpu_ctx, oracle, view):
    import torch
    w, h, bs, cost, maxd, seed = WORKLOADS["config3"]
    left, right, _ = make_pair(w, h, maxd, seed)
    p = wslib.make_params(_view(wslib, view), bs, 0, maxd, 1.0, cost)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    to = torch.empty((h, w), dtype=torch.float32, device="cuda")
    gpu_ctx.search_device(p, tl, tr, to, None)
    torch.cuda.synchronize()
    info = gpu_ctx.last_launch()
    assert info["kernel"] == "ws_march_kernel<sad,%dx%d,halo>" % ((bs, bs) if view == "left" else (bs - 1, bs - 1)), info
    got = to.cpu().numpy().astype(np.float64)
    _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost=cost), ("config3", view))


def test_config5_subpixel_whole_map(wslib, gpu_ctx, oracle):
    """3840 x 2160, 9x9 SSD, D = 1024 in the plan's d-group passes: the integer map is the exact argmin at every pixel,
    the refined one within 1e-4 of the reference's parabola and equal to its float32 rounding."""
    w, h, bs, cost, maxd, seed = WORKLOADS["config5"]
    left, right, _ = make_pair(w, h, maxd, seed)
    p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, maxd, 1.0, cost)
    assert wslib.plan(p, left.shape, right.shape)["passes"] == 4
    whole = _search(wslib, gpu_ctx, "left", left, right, bs, 0, maxd, cost)
    sub = _search(wslib, gpu_ctx, "left", left, right, bs, 0, maxd, cost, subpixel=True)
    assert "march" in gpu_ctx.last_launch()["kernel"]
    want_int = oracle.fast_left(left, right, bs, 0, maxd, cost=cost)
    want_sub = oracle.fast_left(left, right, bs, 0, maxd, cost=cost, subpixel=True)
    _assert_same(whole, want_int, "config5 integer")
    err = np.abs(sub - want_sub).max()
    assert err <= SUBPIXEL_TOL, err
    _assert_same(sub, oracle.fast_left(left, right, bs, 0, maxd, cost=cost, subpixel="float32"), "config5 float32")
    # the refined map's integer part is the argmin, recovered with the reference's fraction
    assert np.array_equal(np.round(sub - (want_sub - want_int)), want_int)


def test_config4_training_h_whole_maps_through_the_batched_host_path(wslib, gpu_ctx, oracle):
    bs = 7
    pairs = [make_pair(w, h, 256, 100 + i) for i, (_n, w, h, _d) in enumerate(TRAINING_H)]
    p = wslib.make_params(wslib.VIEW_LEFT, bs, 0, 256, 1.0, "ssd")
    many = gpu_ctx.search_many(p, [(l, r) for l, r, _ in pairs], dtype=np.float32)
    for (name, w, h, _), (l, r, _), got in zip(TRAINING_H, pairs, many):
        _assert_same(got.astype(np.float64), oracle.fast_left(l, r, bs, 0, 256, cost="ssd"), name)


def test_motorcycle_e_shaped_unequal_pair_whole_maps(wslib, gpu_ctx, oracle):
    w1, h1, w2, h2, maxd = 1481, 1038, 1495, 1052, 140
    left, right, _ = make_pair(w1, h1, maxd, 31, right_width=w2, right_height=h2)
    left[:, :30] = 0
    left[:12] = 0
    right[:, w2 - 40:] = 0
    right[h2 - 20:] = 0
    got = _search(wslib, gpu_ctx, "left", left, right, 7, 0, maxd, "ssd")
    _assert_same(got, oracle.fast_left(left, right, 7, 0, maxd, cost="ssd"), "left")
    for view in ("left", "right"):      # swapped roles: both views legal
        got = _search(wslib, gpu_ctx, view, right, left, 7, 0, maxd, "sad")
        _assert_same(got, _fast(oracle, view)(right, left, 7, 0, maxd, cost="sad"), ("swapped", view))


def test_reference_pipeline_call_at_middlebury_h_size(wslib, gpu_ctx, oracle):
    """main.cpp:40, computeDisparityMapRight(17, 0, 200, 0.9), on a Motorcycle-sized pair (1482 x 994): every row."""
    left, right, _ = make_pair(1482, 994, 200, seed=13)
    got = wslib.BlockSearch(left, right, 17, 0, 200, context=gpu_ctx).computeDisparityMapRight(0.9)
    assert "march" in gpu_ctx.last_launch()["kernel"]
    _assert_same(got, oracle.fast_right(left, right, 17, 0, 200, smooth=0.9), "pipeline call")


@pytest.mark.parametrize("smooth", [0.9, 1.4])
def test_left_view_smooth_raster_bands_whole_map(wslib, gpu_ctx, oracle, smooth):
    """900 x 750: the left view's smoothFactor pass runs in row bands handing their last row down."""
    left, right, _ = make_pair(900, 750, 200, seed=14)
    got = wslib.BlockSearch(left, right, 7, 0, 200, context=gpu_ctx).computeDisparityMapLeft(smooth)
    _assert_same(got, oracle.fast_left(left, right, 7, 0, 200, smooth=smooth), ("left smooth", smooth))


# ---- 2. plan-driven seam sweep --------------------------------------------------------------------------------------
def _plan(wslib, view, bs, cost, maxd, w, h):
    return wslib.plan(wslib.make_params(_view(wslib, view), bs, 0, maxd, 1.0, cost), (h, w, 3), (h, w, 3))


def _family(p):
    if not p["marching"]:
        return "generic"
    if p["tile_cols"] == (p["x_runs"] - 1) * p["x_per_thread"]:
        return "halo"
    return "march%d" % p["d_per_thread"]


def _kernel_ok(family, view, bs, cost, name):
    if family == "generic":
        return name == "ws_generic_kernel"
    ww = bs if view == "left" else bs - 1
    base = "ws_march_kernel<%s,%dx%d" % (cost, ww, ww)
    return name == {"march8": base + ">", "march4": base + ",nd4>", "halo": base + ",halo>"}[family]


def _last_rows(p):
    out_h = p["interior_y1"] - p["interior_y0"]
    return out_h - (p["strips"] - 1) * p["strip_rows"]


def _last_cols(p):
    out_w = p["interior_x1"] - p["interior_x0"]
    return out_w - (p["tiles"] - 1) * p["tile_cols"]


# family name: view, window, cost, the D values the finder may use, the widths it scans heights at (strip seams),
# the height it scans widths at (tile seams)
FAMILIES = {
    "march8": ("left", 7, "ssd", (512,), (400, 600), 120),
    "march4": ("left", 5, "sad", (64,), (300, 400), 120),
    "halo_sad_left": ("left", 9, "sad", (512,), (1200, 1000), 400),
    "halo_sad_right": ("right", 9, "sad", (512,), (1200, 1000), 400),
    "halo_ssd": ("left", 9, "ssd", (512,), (400, 800), 120),
    "centred13": ("left", 13, "ssd", (512,), (400,), 120),
    "centred17": ("right", 17, "ssd", (512,), (400,), 120),
    "plain_sad": ("left", 11, "sad", (512,), (400,), 120),
    "ring_right": ("right", 7, "ssd", (512,), (400, 600), 120),
}
EXPECT = {"march8": "march8", "march4": "march4", "halo_sad_left": "halo", "halo_sad_right": "halo", "halo_ssd": "halo",
          "centred13": "march8", "centred17": "march4", "plain_sad": "march8", "ring_right": "march8"}


def _find(wslib, fam, seam):
    """A shape for family `fam` whose plan puts the image edge on `seam`; fails if the planner no longer gives one."""
    view, bs, cost, ds, widths, tile_h = FAMILIES[fam]
    for maxd in ds:
        for w0 in widths:
            if seam.startswith("strip"):
                scan = [(w0, h) for h in range(bs + 8, 700)]
            else:
                scan = [(w, tile_h) for w in range(maxd + 2 * bs + 8, maxd + 1300)]
            for w, h in scan:
                p = _plan(wslib, view, bs, cost, maxd, w, h)
                if _family(p) != EXPECT[fam]:
                    continue
                if seam.startswith("strip"):
                    if p["strips"] < 2 or p["strip_rows"] < 3:
                        continue
                    want = 1 if seam == "strip_1" else p["strip_rows"] - 1
                    if _last_rows(p) == want:
                        return w, h, maxd, p
                else:
                    if p["tiles"] < 2 or p["tile_cols"] < 3:
                        continue
                    want = 1 if seam == "tile_1" else p["tile_cols"] - 1
                    if _last_cols(p) == want:
                        return w, h, maxd, p
    pytest.fail("the planner gives family %s no shape with seam %s" % (fam, seam))


def _run_case(wslib, ctx, oracle, view, bs, cost, maxd, w, h, family, seed, what):
    left, right, _ = make_pair(w, h, maxd, seed)
    left[h // 2, w // 3:w // 3 + 5] = 0                  # a few black pixels on each side
    right[h // 3, w // 2:w // 2 + 5] = 0
    got = _search(wslib, ctx, view, left, right, bs, 0, maxd, cost)
    name = ctx.last_launch()["kernel"]
    assert _kernel_ok(family, view, bs, cost, name), (what, family, name)
    _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost=cost), what)


@pytest.mark.parametrize("seam", ["strip_1", "strip_m1", "tile_1", "tile_m1"])
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_seam_sweep(wslib, gpu_ctx, oracle, fam, seam):
    view, bs, cost = FAMILIES[fam][:3]
    w, h, maxd, p = _find(wslib, fam, seam)
    if fam.startswith("centred"):                        # the centred SSD key layout (ssd_needs_centring, ws_device.h)
        ww = bs if view == "left" else bs - 1
        assert 2 * ww * ww * 3 * 255 * 255 * p["d_per_thread"] >= 1 << 28, p
        assert (255 * 255 - 127 * 127) * ww * ww * 3 * p["d_per_thread"] < 1 << 28, p
    _run_case(wslib, gpu_ctx, oracle, view, bs, cost, maxd, w, h, EXPECT[fam], 600 + len(fam) + len(seam),
              (fam, seam, w, h, maxd, p))


@pytest.mark.parametrize("bs", [19, 21])
@pytest.mark.parametrize("view", ["left", "right"])
def test_brute_force_fallback_whole_map(wslib, gpu_ctx, oracle, view, bs):
    for cost, (w, h, maxd) in (("ssd", (157, 41, 40)), ("sad", (230, 33, 300))):
        assert _family(_plan(wslib, view, bs, cost, maxd, w, h)) == "generic"
        _run_case(wslib, gpu_ctx, oracle, view, bs, cost, maxd, w, h, "generic", bs, (view, bs, cost))


@pytest.mark.parametrize("fam", ["march8", "halo_ssd", "plain_sad", "march4"])
def test_d_at_whole_chunks_and_either_side(wslib, gpu_ctx, oracle, fam):
    """D = passes x d_chunks x d_per_thread exactly (every chunk full), and one either side (one chunk one short, one
    chunk holding a single disparity)."""
    view, bs, cost, ds, widths, _ = FAMILIES[fam]
    w, h = widths[0], 60
    found = None
    for maxd in range(ds[0], 8, -1):
        p = _plan(wslib, view, bs, cost, maxd, w, h)
        if _family(p) == EXPECT[fam] and p["passes"] * p["d_chunks"] * p["d_per_thread"] == maxd:
            found = maxd
            break
    assert found, fam
    for maxd in (found - 1, found, found + 1):
        p = _plan(wslib, view, bs, cost, maxd, w, h)
        family = _family(p)
        assert family.startswith("march") or family == "halo", p
        _run_case(wslib, gpu_ctx, oracle, view, bs, cost, maxd, w, h, family, maxd, (fam, maxd, p))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_pass_count_steps(wslib, gpu_ctx, oracle, view, cost):
    """Both sides of every D where the plan's d-group pass count changes, up to D = 1640: from one pass to several
    (the key plane appears) and, for SSD, from 3 to 4 passes."""
    bs, w, h = 7, 1700, 14
    passes = {}
    for maxd in range(400, 1640):
        passes[maxd] = _plan(wslib, view, bs, cost, maxd, w, h)["passes"]
    steps = [d for d in range(401, 1640) if passes[d - 1] != passes[d]]
    assert steps and passes[steps[0] - 1] == 1 and passes[steps[0]] >= 2, steps
    if cost == "ssd":
        assert any(passes[d - 1] == 3 and passes[d] == 4 for d in steps), [(d, passes[d - 1], passes[d]) for d in steps]
    for step in steps:
        for maxd in (step - 1, step):
            p = _plan(wslib, view, bs, cost, maxd, w, h)
            _run_case(wslib, gpu_ctx, oracle, view, bs, cost, maxd, w, h, _family(p), maxd, (view, cost, maxd, p))


@pytest.mark.parametrize("view", ["left", "right"])
def test_d_clamped_by_the_width(wslib, gpu_ctx, oracle, view):
    for bs, cost, w in ((7, "ssd", 90), (9, "sad", 131), (5, "sad", 300)):
        p = _plan(wslib, view, bs, cost, 3 * w, w, 40)
        assert p["marching"], p
        _run_case(wslib, gpu_ctx, oracle, view, bs, cost, 3 * w, w, 40, _family(p), w, (view, bs, cost))


# ---- 3. key-range extremes ------------------------------------------------------------------------------------------
P_HI = np.array([255, 0, 255], np.uint8)     # neither pixel is black, every channel differs by 255:
P_LO = np.array([0, 255, 0], np.uint8)       # the largest pixel cost there is, SSD and SAD


def _extreme_pair(w, h, kind, rng):
    left = np.broadcast_to(P_HI, (h, w, 3)).copy()
    right = np.broadcast_to(P_LO, (h, w, 3)).copy()
    if kind == "one_below":                  # one pixel of the right image one unit closer: its windows cost max - 1
        for _ in range(3):                   # (SAD; SSD: max - 509), so those candidates win
            y, x = int(rng.integers(h)), int(rng.integers(w))
            right[y, x, 1] = 254
            left[int(rng.integers(h)), int(rng.integers(w)), 0] = 254
    elif kind == "columns":                  # alternating columns: every other candidate costs 0, the rest the maximum
        left[:, 1::2] = P_LO
        right[:, 1::2] = P_HI
    return left, right


MARCH_WINDOWS = [3, 5, 7, 9, 11, 13, 15, 17]          # WS_MARCH_TABLE: left bs x bs, right (bs - 1) x (bs - 1)


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_maximum_cost_windows(wslib, gpu_ctx, oracle, view, cost):
    rng = np.random.default_rng(1 if view == "left" else 2)
    for bs in MARCH_WINDOWS:
        for kind in ("all_max", "one_below", "columns"):
            for w, h, maxd in ((3 * bs + 40, bs + 6, 2 * bs + 20), (700, bs + 3, 600)):     # 1 pass; several
                left, right = _extreme_pair(w, h, kind, rng)
                got = _search(wslib, gpu_ctx, view, left, right, bs, 0, maxd, cost)
                p = _plan(wslib, view, bs, cost, maxd, w, h)
                assert _kernel_ok(_family(p), view, bs, cost, gpu_ctx.last_launch()["kernel"]), (bs, kind, p)
                assert p["marching"] or (cost == "sad" and bs >= 11), (bs, kind, p)
                _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost=cost), (view, cost, bs, kind, maxd))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("bs", MARCH_WINDOWS)
def test_maximum_cost_at_the_last_d_the_marching_kernel_accepts(wslib, gpu_ctx, oracle, view, bs):
    """Plain (unpacked) SAD keys are cost << tag bits below 2^28 (march_supported): the largest D the planner still
    marches and the first it refuses, both with windows at the maximum cost.  SSD and packed SAD do not refuse by D
    within an image's width; for them the widest D of the image is run."""
    rng = np.random.default_rng(bs)
    for cost in ("sad", "ssd"):
        h = bs + 3
        wmax = 2600
        ok = [d for d in (64, 128, 256, 512, 1024, 2048) if _plan(wslib, view, bs, cost, d, wmax, h)["marching"]]
        if not ok:
            continue
        lo = ok[-1]
        hi = lo * 2
        if _plan(wslib, view, bs, cost, min(hi, wmax - bs - 2), wmax, h)["marching"]:
            ds = [wmax - bs - 2]                             # no refusal in reach
        else:
            while hi - lo > 1:                               # the boundary, by probing the plan
                mid = (lo + hi) // 2
                if _plan(wslib, view, bs, cost, mid, wmax, h)["marching"]:
                    lo = mid
                else:
                    hi = mid
            ds = [lo, hi]
            assert _plan(wslib, view, bs, cost, lo, wmax, h)["marching"] and not _plan(wslib, view, bs, cost, hi, wmax, h)["marching"]
        for maxd in ds:
            w = min(wmax, maxd + bs + 24)
            left, right = _extreme_pair(w, h, "one_below", rng)
            got = _search(wslib, gpu_ctx, view, left, right, bs, 0, maxd, cost)
            p = _plan(wslib, view, bs, cost, maxd, w, h)
            assert _kernel_ok(_family(p), view, bs, cost, gpu_ctx.last_launch()["kernel"]), (cost, maxd, p)
            _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost=cost), (view, cost, bs, maxd))


@pytest.mark.parametrize("view", ["left", "right"])
def test_centred_ssd_16_and_17_wide_windows_at_maximum_contrast(wslib, gpu_ctx, oracle, view):
    """Regression: a centred SSD key is (sum b^2 - 2 sum a.b) << log2(nd), whose top per channel is 255^2 - 127^2 (a
    reference 255 against a target 0), not the 2 * 128^2 march_supported used to assume.  With 8 disparities per thread
    the 16 x 16 (right view, bs 17) and 17 x 17 (left view) windows then passed 2^28 at high contrast and their pixels
    came out as 'no candidate'.  The planner now gives those windows 4 disparities per thread.  The shape is one where
    the cost model prefers 8."""
    rng = np.random.default_rng(17)
    bs, w, h, maxd = 17, 400, 116, 512
    p = _plan(wslib, view, bs, "ssd", maxd, w, h)
    ww = bs if view == "left" else bs - 1
    assert p["marching"] and p["d_per_thread"] == 4, p
    assert (255 * 255 - 127 * 127) * ww * ww * 3 * p["d_per_thread"] < 1 << 28
    for kind in ("all_max", "one_below", "columns"):
        left, right = _extreme_pair(w, h, kind, rng)
        got = _search(wslib, gpu_ctx, view, left, right, bs, 0, maxd, "ssd")
        assert gpu_ctx.last_launch()["kernel"] == "ws_march_kernel<ssd,%dx%d,nd4>" % (ww, ww)
        _assert_same(got, _fast(oracle, view)(left, right, bs, 0, maxd, cost="ssd"), (view, kind))


@pytest.mark.parametrize("smooth", [1.0, 0.9])
@pytest.mark.parametrize("view", ["left", "right"])
def test_largest_window_at_maximum_contrast(wslib, gpu_ctx, oracle, view, smooth):
    """bs 63, the largest the ABI accepts: the brute-force kernel, and with smoothFactor 0.9 the smooth path's top-3
    table, whose 'no candidate' word (kTopNone) must stay above every window cost (63 * 63 * 3 * 255^2 < 2^30)."""
    rng = np.random.default_rng(63)
    for cost in ("ssd", "sad"):
        for kind in ("all_max", "one_below", "columns"):
            w, h = 150, 70
            left, right = _extreme_pair(w, h, kind, rng)
            got = _search(wslib, gpu_ctx, view, left, right, 63, 0, 50, cost, smooth=smooth)
            _assert_same(got, _fast(oracle, view)(left, right, 63, 0, 50, smooth=smooth, cost=cost),
                         (view, cost, kind, smooth))
