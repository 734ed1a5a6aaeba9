"""Sub-pixel maps bit for bit: every refined pixel against the fast reference's float32 mode (oracle.fast_left /
fast_right with subpixel="float32", pinned to the slow reference and to a NumPy witness by
tests/test_subpixel_reference.py).

The device stores d + (float)(num / (2.0 * den)) from exact integer costs, so the map is fully determined; a 1e-4
tolerance lets a cost that is wrong by a few units through (the fraction's denominator grows with the window).  Each
case here
  * compares the whole float32 map with np.array_equal against the reference's float32 mode,
  * keeps the 1e-4 bound against the double refinement,
  * checks that the integer part is the integer map (and the device's integer map is the reference's).
The cases reach every form of ws_refine_planes_kernel (SAD, plain and centred SSD; the compile-time widths 7 and 9 and
the generic one; the right view's mirrored layout) after each marching family, ws_refine_kernel (the right view's
border ring, unequal pairs, the brute-force fallback, tiny and ragged images, bs 63), the candidate-range edges, cost
extremes, the full-size configs and every entry point.  Where a case names a kernel form, the plan says it ran.
"""
import numpy as np
import pytest

from stereo_reconstruction_amd.synthetic import make_pair
from test_subpixel_reference import shifted_pair

pytestmark = pytest.mark.gpu

TOL = 1e-4
WORKLOADS = {    # bench.WORKLOADS: (width, height, block, cost, maxD, seed)
    "config2": (1500, 1000, 7, "ssd", 256, 2),
    "config3": (2964, 1988, 9, "sad", 512, 3),
    "config5": (3840, 2160, 9, "ssd", 1024, 5),
}


def _view(wslib, view):
    return wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT


def _fast(oracle, view):
    return oracle.fast_left if view == "left" else oracle.fast_right


def _params(wslib, view, bs, mind, maxd, cost, subpixel=True):
    return wslib.make_params(_view(wslib, view), bs, mind, maxd, 1.0, cost, subpixel=subpixel)


def _family(p):
    if not p["marching"]:
        return "generic"
    if p["tile_cols"] == (p["x_runs"] - 1) * p["x_per_thread"]:
        return "halo"
    return "march%d" % p["d_per_thread"]


def _ww(view, bs):
    return bs if view == "left" else 2 * ((bs - 1) // 2)


def _centred(p, view, bs, cost):
    """ssd_needs_centring(ww, wh, nd) (ws_device.h) with the plan's disparities per thread: the refine then reads the
    centred (byte - 128) planes."""
    ww = _ww(view, bs)
    return cost == "ssd" and 2 * ww * ww * 3 * 255 * 255 * p["d_per_thread"] >= 1 << 28


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %r, want %r)"
                             % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _verify(wslib, ctx, oracle, view, left, right, bs, mind, maxd, cost, got, what):
    """The three comparisons of every case; returns (integer map, refined mask)."""
    fast = _fast(oracle, view)
    want = fast(left, right, bs, mind, maxd, cost=cost, subpixel="float32")
    _assert_same(got, want, ("float32", what))
    dbl = fast(left, right, bs, mind, maxd, cost=cost, subpixel=True)
    err = np.abs(got - dbl).max(initial=0.0)
    assert err <= TOL, (what, err)
    want_int = fast(left, right, bs, mind, maxd, cost=cost)
    got_int = ctx.search(_params(wslib, view, bs, mind, maxd, cost, subpixel=False), left, right)
    _assert_same(got_int, want_int, ("integer", what))
    assert np.abs(got - got_int).max(initial=0.0) <= 0.5, what
    assert np.array_equal(np.round(got - (dbl - want_int)), want_int), what
    return want_int, got != want_int


def _case(wslib, ctx, oracle, view, left, right, bs, mind, maxd, cost, what, family=None, centred=None):
    """Host call, float32 map; asserts the plan's family / refine form when named.  Returns (map, integer map,
    refined mask, plan with the kernel that ran under "kernel")."""
    p = wslib.plan(_params(wslib, view, bs, mind, maxd, cost), left.shape, right.shape)
    if family is not None:
        assert _family(p) == family, (what, p)
    if centred is not None:
        assert p["marching"] and _centred(p, view, bs, cost) == centred, (what, p)
    got = ctx.search(_params(wslib, view, bs, mind, maxd, cost), left, right, dtype=np.float32).astype(np.float64)
    p["kernel"] = ctx.last_launch()["kernel"]
    assert ("march" in p["kernel"]) == bool(p["marching"]), (what, p)
    want_int, refined = _verify(wslib, ctx, oracle, view, left, right, bs, mind, maxd, cost, got, what)
    return got, want_int, refined, p


def _interior(p):
    return (slice(p["interior_y0"], p["interior_y1"]), slice(p["interior_x0"], p["interior_x1"]))


# ---- 1. every form of ws_refine_planes_kernel ------------------------------------------------------------------------
# view, bs, cost, maxD, the plan's family, centred SSD planes; 400 x 116 (the shape of the centred nd4 regression).
# Compile-time widths: left 7 and 9; every right-view window (2 half) and the other left ones take the generic form.
FORMS = [
    ("left", 5, "ssd", 512, "march8", False),
    ("left", 5, "sad", 96, "march4", False),
    ("left", 7, "ssd", 512, "march8", False),
    ("left", 7, "sad", 512, "march8", False),
    ("left", 9, "ssd", 512, "halo", False),
    ("left", 9, "sad", 512, "march8", False),
    ("left", 11, "ssd", 512, "march8", True),
    ("left", 11, "ssd", 96, "march4", False),
    ("left", 11, "sad", 512, "march8", False),
    ("left", 13, "ssd", 512, "march8", True),
    ("left", 13, "ssd", 96, "march4", False),
    ("left", 15, "sad", 512, "march8", False),
    ("left", 17, "ssd", 512, "march4", True),
    ("left", 17, "sad", 512, "march8", False),
    ("right", 8, "ssd", 512, "march8", False),
    ("right", 8, "sad", 512, "march8", False),
    ("right", 9, "ssd", 512, "halo", False),
    ("right", 9, "sad", 512, "march8", False),
    ("right", 11, "ssd", 512, "march8", True),
    ("right", 11, "ssd", 96, "march4", False),
    ("right", 17, "ssd", 512, "march4", True),
    ("right", 17, "sad", 512, "march8", False),
]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%s-bs%d-%s-D%d" % f[:4])
def test_refine_planes_kernel_forms(wslib, gpu_ctx, oracle, form):
    view, bs, cost, maxd, family, centred = form
    w, h = 400, 116
    left, right, _ = make_pair(w, h, min(maxd, 160), 700 + bs + maxd)
    left[h // 2, 100:106] = 0
    right[h // 3, 200:206] = 0
    got, want_int, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, form,
                                      family=family, centred=centred)
    inner = np.zeros_like(refined)
    inner[_interior(p)] = True
    assert refined[inner].mean() > 0.3, (form, refined[inner].mean())
    if view == "right":        # the border ring (ws_refine_kernel): clipped windows, refined pixels there too
        ring = ~inner
        ring[min(left.shape[0], right.shape[0]):] = False
        assert refined[ring].sum() > 50, (form, refined[ring].sum())


@pytest.mark.parametrize("view", ["left", "right"])
def test_centred_nd4_plans_at_maximum_contrast(wslib, gpu_ctx, oracle, view):
    """The 4-disparities-per-thread centred SSD plans of test_centred_ssd_16_and_17_wide_windows_at_maximum_contrast
    (bs 17, 400 x 116, D = 512), on a maximum-contrast pair: every pixel 255/0/255 or 0/255/0, a true disparity and
    a few flipped pixels, so that the costs and den are as large as these windows allow and a wrong cost moves the
    fraction by far less than 1e-4."""
    bs, w, h, maxd = 17, 400, 116, 512
    left, right = _max_contrast_pair(w, h, 37, seed=17)
    _, want_int, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, "ssd", (view, "nd4"),
                                    family="march4", centred=True)
    assert p["d_per_thread"] == 4 and refined.sum() > 1000, (p, refined.sum())


# ---- 2. after each marching family -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [("march8", "left", 7, "ssd", 512, 400, 120), ("march4", "left", 5, "sad", 64, 300, 120),
                                 ("halo", "left", 9, "ssd", 512, 400, 120), ("march8", "left", 11, "sad", 512, 400, 120),
                                 ("halo", "left", 9, "sad", 512, 1200, 400), ("halo", "right", 9, "sad", 512, 1200, 400)],
                         ids=["march8", "march4", "halo_ssd", "plain_sad", "halo_sad_left", "halo_sad_right"])
def test_after_each_marching_family(wslib, gpu_ctx, oracle, fam):
    family, view, bs, cost, maxd, w, h = fam
    left, right, _ = make_pair(w, h, maxd, 650 + bs + w)
    _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, fam, family=family)
    assert refined.mean() > 0.3
    if family == "halo" and cost == "sad":
        ww = _ww(view, bs)
        assert p["kernel"] == "ws_march_kernel<sad,%dx%d,halo>" % (ww, ww), p


# ---- 3. ws_refine_kernel: what the marching interior does not hold ----------------------------------------------------
@pytest.mark.parametrize("shapes", [(300, 80, 290, 70), (290, 70, 300, 80), (300, 70, 300, 71)],
                         ids=["taller_left", "taller_right", "right_one_row_taller"])
def test_unequal_pairs(wslib, gpu_ctx, oracle, shapes):
    """Either image taller / wider: rows past min(h1, h2) (zeros), and the refine's row / column limits.  The right view
    takes a right image taller than the left one only where no window needs a left row >= h1 (h2 = h1 + 1, bs 7; any
    height for bs <= 4)."""
    w1, h1, w2, h2 = shapes
    left, right, _ = make_pair(w1, h1, 40, 60 + h2, right_width=w2, right_height=h2)
    for view, bs, cost in (("left", 7, "ssd"), ("left", 9, "sad"), ("right", 7, "ssd"), ("right", 3, "sad")):
        if view == "right" and h2 > h1 + 1 and bs > 4:
            continue
        got, _, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 40, cost, (shapes, view, bs))
        assert refined.any()
        assert (got[min(h1, h2):] == 0).all()
    _, tall, _ = make_pair(w1, h1, 40, 61, right_width=w1, right_height=h1 + 2)
    with pytest.raises(wslib.WsError) as e:      # two extra rows: a bs 7 window leaves the left image
        gpu_ctx.search(_params(wslib, "right", 7, 0, 40, "ssd"), left, tall)
    assert e.value.code == -2


@pytest.mark.parametrize("bs", [19, 21])
@pytest.mark.parametrize("view", ["left", "right"])
def test_brute_force_fallback_shapes(wslib, gpu_ctx, oracle, view, bs):
    for cost, (w, h, maxd) in (("ssd", (157, 41, 40)), ("sad", (230, 33, 300))):
        left, right, _ = make_pair(w, h, min(maxd, 60), bs + w)
        _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, (view, bs, cost),
                                 family="generic")
        assert p["kernel"] == "ws_generic_kernel" and refined.any(), p


def test_tiny_and_ragged_images(wslib, gpu_ctx, oracle):
    rng = np.random.default_rng(31)
    n = 0
    for w, h in ((1, 1), (2, 2), (3, 5), (5, 3), (9, 9), (17, 4), (31, 17), (257, 19), (263, 33), (129, 65)):
        left = rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8)
        right = rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8)
        if w > 8:
            left, right, _ = make_pair(w, h, 8, w + h)
        for view in ("left", "right"):
            for bs, cost in ((3, "ssd"), (5, "sad"), (7, "ssd")):
                _, _, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, w + 3, cost, (w, h, view, bs))
                n += int(refined.sum())
    assert n > 1000, n


@pytest.mark.parametrize("view", ["left", "right"])
def test_largest_window(wslib, gpu_ctx, oracle, view):
    """bs 63, the largest the ABI accepts (the brute-force kernel)."""
    left, right, _ = make_pair(150, 70, 40, 63)
    for cost in ("ssd", "sad"):
        _, _, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, 63, 0, 50, cost, (view, cost),
                                 family="generic")
        assert refined.any()


# ---- 4. candidate-range edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["left", "right"])
def test_min_disparity_and_tiny_ranges(wslib, gpu_ctx, oracle, view):
    """minD > 0 (the left view ignores it; the right view's d - 1 must still be >= minD), maxD 2 and 3 (nothing /
    only the middle candidate refined), a range far wider than the image."""
    left, right, _ = make_pair(300, 40, 48, 71)
    for bs, cost in ((7, "ssd"), (9, "sad")):
        for mind, maxd in ((5, 48), (20, 40)):
            _, want_int, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, mind, maxd, cost,
                                            (view, bs, mind, maxd))
            assert refined.any()
            if view == "right":
                assert (want_int[refined] > mind).all()
        for maxd in (2, 3):
            t = 2 if view == "left" else 1
            l2, r2 = shifted_pair(200, 40, t, seed=maxd + bs)
            _, want_int, refined, _ = _case(wslib, gpu_ctx, oracle, view, l2, r2, bs, 0, maxd, cost, (view, bs, maxd))
            assert refined.any() == (maxd == 3), (view, bs, maxd)
        _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 3000, cost, (view, bs, 3000))
        assert p["marching"] and refined.any()


def test_right_view_negative_min_disparity_is_refused(wslib, gpu_ctx, oracle):
    left, right, _ = make_pair(120, 30, 20, 72)
    for mind in (-1, -7):
        with pytest.raises(wslib.WsError) as e:
            gpu_ctx.search(_params(wslib, "right", 7, mind, 20, "ssd"), left, right)
        assert e.value.code == -2
        with pytest.raises(oracle.OracleGeometryError):
            oracle.fast_right(left, right, 7, mind, 20, subpixel="float32")


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_both_sides_of_a_pass_count_change(wslib, gpu_ctx, oracle, view, cost):
    """The first D where the plan goes from one d-group pass to several (the key plane appears) and, for SSD, from 3 to
    4 passes: the refine reads the winner the passes agreed on."""
    bs, w, h = 7, 1700, 14
    passes = {d: wslib.plan(_params(wslib, view, bs, 0, d, cost), (h, w, 3), (h, w, 3))["passes"] for d in range(400, 1640)}
    steps = [d for d in range(401, 1640) if passes[d - 1] != passes[d]]
    assert steps and passes[steps[0] - 1] == 1
    picked = [steps[0]] + ([d for d in steps if passes[d - 1] == 3 and passes[d] == 4][:1] if cost == "ssd" else [])
    assert len(picked) == (2 if cost == "ssd" else 1), steps
    for step in picked:
        for maxd in (step - 1, step):
            left, right, _ = make_pair(w, h, 300, maxd)
            _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, (view, cost, maxd))
            assert p["passes"] == passes[maxd] and refined.any()


@pytest.mark.parametrize("view", ["left", "right"])
def test_winners_at_the_range_edges(wslib, gpu_ctx, oracle, view):
    """Shifted copies whose true disparity is 1, 2, maxD - 1 or maxD - 2: winners on an end of the candidate range
    (left 1 and maxD, right 0 and maxD - 1) are not refined, one step inside they are."""
    maxd, w, h = 64, 300, 48
    lo, hi = (1, maxd) if view == "left" else (0, maxd - 1)
    for bs, cost in ((7, "ssd"), (9, "sad")):
        for t in (1, 2, maxd - 1, maxd - 2):
            left, right = shifted_pair(w, h, t, seed=t * 3 + bs)
            _, want_int, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, (view, bs, t))
            at_t = want_int == t
            assert at_t.sum() > 1000, (view, bs, t, at_t.sum())
            assert refined[at_t].any() == (t not in (lo, hi)), (view, bs, t)


# ---- 5. cost extremes ------------------------------------------------------------------------------------------------
P_HI = np.array([255, 0, 255], np.uint8)
P_LO = np.array([0, 255, 0], np.uint8)


def _max_contrast_pair(w, h, t, seed):
    """Every pixel P_HI or P_LO (each channel 0 or 255, never black), R(y, x) = L(y, x + t), 2 % of the pixels
    flipped in each image: window costs in multiples of the largest pixel cost."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(h, w + t))
    base = np.where(bits[..., None] == 1, P_HI, P_LO)
    left, right = base[:, :w].copy(), base[:, t:t + w].copy()
    for img in (left, right):
        flip = rng.random(img.shape[:2]) < 0.02
        img[flip] = np.where((img[flip] == P_HI).all(axis=1)[:, None], P_LO, P_HI)
    return left, right


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_maximum_contrast_at_the_largest_marching_windows(wslib, gpu_ctx, oracle, view, cost):
    """17 x 17 (left) and 16 x 16 (right), the largest windows the marching kernel takes, and 9 x 9: den is as large as
    these windows make it."""
    for bs, maxd in ((17, 128), (9, 128), (17, 40)):
        left, right = _max_contrast_pair(360, 64, 23, seed=bs + maxd)
        _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, (view, cost, bs, maxd))
        assert p["marching"] and refined.sum() > 1000, (p, refined.sum())


@pytest.mark.parametrize("view", ["left", "right"])
def test_constant_and_two_level_images(wslib, gpu_ctx, oracle, view):
    """Constant images: every candidate ties, the winner sits on the end of its range, the map is the integer map.
    Two- and three-level images in flat blocks: ties beside refined pixels."""
    for cost in ("ssd", "sad"):
        for bs in (5, 9):
            left, right = np.full((40, 160, 3), 90, np.uint8), np.full((40, 160, 3), 70, np.uint8)
            got, want_int, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 30, cost, (view, cost, bs))
            assert not refined.any() and np.array_equal(got, want_int)
            for levels in (2, 3):
                left, right = shifted_pair(160, 40, 5, seed=levels + bs, noise=0, levels=levels, block=6)
                got, want_int, refined, _ = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 30, cost,
                                                  (view, cost, bs, levels))
                assert refined.any() and (~refined).sum() > 100


# ---- 6. full size ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("config2", "left"), ("config2", "right"), ("config5", "right"),
                                  ("config3", "left"), ("config3", "right")], ids=lambda c: "%s-%s" % c)
def test_full_size(wslib, gpu_ctx, oracle, case):
    name, view = case
    w, h, bs, cost, maxd, seed = WORKLOADS[name]
    left, right, _ = make_pair(w, h, maxd, seed)
    family = "halo" if name == "config3" else None
    _, _, refined, p = _case(wslib, gpu_ctx, oracle, view, left, right, bs, 0, maxd, cost, case, family=family)
    assert p["marching"] and refined.mean() > 0.5, (p, refined.mean())


# ---- 7. entry points -------------------------------------------------------------------------------------------------
def test_entry_points(wslib, gpu_ctx, oracle):
    """Host float32 (the other cases), host float64 (the float32 map widened), the device entry into a torch tensor,
    the batched host path."""
    import torch
    pairs = [make_pair(320, 90, 48, 80 + i) for i in range(3)]
    for view, bs, cost in (("left", 7, "ssd"), ("right", 9, "sad"), ("left", 13, "ssd")):
        p = _params(wslib, view, bs, 0, 48, cost)
        for left, right, _ in pairs[:1]:
            f32 = gpu_ctx.search(p, left, right, dtype=np.float32)
            f64 = gpu_ctx.search(p, left, right, dtype=np.float64)
            assert f64.dtype == np.float64 and np.array_equal(f64, f32.astype(np.float64)), (view, bs)
            _verify(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 48, cost, f64, ("host f64", view, bs))
            tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            to = torch.full(f32.shape, -7.0, dtype=torch.float32, device="cuda")
            gpu_ctx.search_device(p, tl, tr, to, None, check=True)
            torch.cuda.synchronize()
            dev = to.cpu().numpy().astype(np.float64)
            _verify(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 48, cost, dev, ("device", view, bs))
        for dtype in (np.float32, np.float64):
            many = gpu_ctx.search_many(p, [(l, r) for l, r, _ in pairs], dtype=dtype)
            for k, ((left, right, _), got) in enumerate(zip(pairs, many)):
                assert got.dtype == dtype
                _verify(wslib, gpu_ctx, oracle, view, left, right, bs, 0, 48, cost, got.astype(np.float64),
                        ("search_many", view, bs, dtype.__name__, k))
