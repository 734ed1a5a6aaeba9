"""smoothFactor != 1, whole maps, every pixel, against the fast exact CPU reference (oracle.fast_left / fast_right, pinned
to the line-cited oracle by tests/test_fast_reference.py) and oracle.linear for LinearSearch.

ws_smooth.hip chooses among many kernel forms by width, height, factor, window and D; every case here names the form
its shape is for (derived from the launch arithmetic, not hard-coded), and puts the image edge on the seam it is about:
  * right view / LinearSearch resolvers: the chunked wave resolvers <8|16|32> (one chunk, one either side, three or
    more chunks), the 1024-thread resolver (width above 2048, or above 3968 for 0 <= s <= 1), the bit-plane resolvers
    <1|2> (widths 1985-3968 take two 31-column words per lane), each once at a full Middlebury / 4K height;
  * right-view prepare on the marching kernel's planes (box + ring: SAD, plain SSD, centred SSD) at the box-tile
    seams, with a multi-pass D, and the generic prepare for windows without a marching kernel;
  * the left view's raster bands: every reachable ws_smooth_left_bands_kernel<MODE, BS, TW>, D either side of the LDS
    limits, interior heights at 32-row band seams, D at the top-3 table's 8-disparity slab boundaries;
  * the batched host path, two streams with growing scratch, float32 and float64 host outputs.
In the right view and LinearSearch the factor only reaches d = 0 beside a neighbour whose stored value is 0, which
textured pairs almost never give.  _scene therefore adds a periodic few-level texture (d = 0, p, 2p, ... tie up to
noise), a noise-free patch (exact ties) and black columns (vertical zero runs through every row seam).  Every case
asserts that the reference map at s differs from the one at s = 1, and for a seam case on both sides of the seam.
Integer maps are compared with np.array_equal.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from stereo_reconstruction_amd.synthetic import TRAINING_H, make_pair
from test_gpu_whole_map import WORKLOADS, _assert_same, _view

pytestmark = pytest.mark.gpu

INF = float("inf")


# ---- scenes and cached references -----------------------------------------------------------------------------------
# (bounded: a pair and its maps are shared by the cases of one test and by neighbouring tests, not by the whole
# session -- full-size float64 maps are 35-70 MB each; the module's teardown drops what is left)
@functools.lru_cache(maxsize=6)
def _scene(w, h, maxd, seed, rw=None, rh=None, period=7, edge_black=None):
    """make_pair with, in columns [w/4, w/2) of both images, a texture of period `period` on four levels plus
    independent noise of 0..3 (candidates d = 0, p, 2p, ... cost nearly the same), a noise-free patch of it (exact
    ties) and four black columns (the map is 0 there: zero runs through every row).  edge_black: the texture starts at
    column 0 instead, and a black column at that x with no other within 3 columns of it."""
    left, right, _ = make_pair(w, h, maxd, seed, right_width=rw, right_height=rh)
    rng = np.random.default_rng(seed + 7919)
    tile = (rng.integers(0, 4, size=(max(left.shape[0], right.shape[0]), period, 3)) * 50 + 30).astype(np.int16)
    for img in (left, right):
        ih, iw = img.shape[:2]
        x0, x1 = (iw // 4 if edge_black is None else 0), iw // 2
        tex = tile[:ih][:, np.arange(x0, x1) % period]
        img[:, x0:x1] = (tex + rng.integers(0, 4, size=tex.shape)).astype(np.uint8)
        py0 = ih // 3
        pw = max(0, min(60, x1 - x0 - 12))
        img[py0:py0 + 40, x0 + 10:x0 + 10 + pw] = tex[py0:py0 + 40, 10:10 + pw].astype(np.uint8)
        black = [(x0 + x1) // 2, (2 * iw) // 3, iw - 5]
        if edge_black is None:
            black.append(x0 + 3)
        else:                                   # (one lone zero run there: the columns beside it are the point)
            black = [x for x in black if abs(x - edge_black) > 3] + [edge_black]
        img[:, black] = 0
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=8)
def _ref(view, key, bs, mind, maxd, s, cost):
    left, right = _scene(*key)
    if view == "linear":
        return oracle_mod().linear(left, right, s, maxd, threads=oracle_mod().host_threads())
    f = oracle_mod().fast_left if view == "left" else oracle_mod().fast_right
    return f(left, right, bs, mind, maxd, smooth=s, cost=cost)


def oracle_mod():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _ref.cache_clear()
    _scene.cache_clear()


def _run(wslib, ctx, view, key, bs, mind, maxd, s, cost="ssd", dtype=np.float64):
    left, right = _scene(*key)
    if view == "linear":
        p = wslib.make_params(wslib.VIEW_LINEAR, 1, 0, maxd, s, "ssd", linear_range=maxd)
    else:
        p = wslib.make_params(_view(wslib, view), bs, mind, maxd, s, cost)
    return ctx.search(p, left, right, dtype=dtype)


def _check(wslib, ctx, view, key, bs, mind, maxd, s, cost="ssd", rows=(), cols=(), what=None):
    """Run one case against the reference; the factor must matter (somewhere, and in every row / column named)."""
    want = _ref(view, key, bs, mind, maxd, s, cost)
    want1 = _ref(view, key, bs, mind, maxd, 1.0, cost)
    what = what or (view, key, bs, mind, maxd, s, cost)
    assert not np.array_equal(want, want1), ("the factor is idle", what)
    for r in rows:
        assert (want[r] != want1[r]).any(), ("the factor is idle in row %d" % r, what)
    for c in cols:
        assert (want[:, c] != want1[:, c]).any(), ("the factor is idle in column %d" % c, what)
    got = _run(wslib, ctx, view, key, bs, mind, maxd, s, cost)
    _assert_same(got, want, what)
    return got


# The right view's smoothFactor path runs its data-parallel search (the marching kernel, whose planes and cost plane
# the prepare kernels read) with min_disparity 1: d = 0 is decided by the prepare / resolve passes (search_on,
# ws_search.cpp).  The plan of that launch is the plan with mind = SMOOTH_RIGHT_MIND.
SMOOTH_RIGHT_MIND = 1


def _plan(wslib, view, bs, cost, maxd, w, h, mind=0, rw=None, rh=None):
    return wslib.plan(wslib.make_params(_view(wslib, view), bs, mind, maxd, 1.0, cost), (h, w, 3),
                      ((rh or h), (rw or w), 3))


# ---- right view / LinearSearch resolvers (launch_smooth) ------------------------------------------------------------
BITS_MAX1, BITS_MAX2 = 31 * 64, 62 * 64          # kBitsMaxWidth1 / 2: 31-column words, one or two per lane


def _chunk(w2):
    """Rows per LDS chunk of the wave resolvers: two chunks in 64 KB, a multiple of 16, at most 64."""
    sel_pitch = (w2 + 63) & ~63
    return min(64, (32768 // sel_pitch) // 16 * 16)


def _resolver(w2, s):
    if 0.0 <= s <= 1.0 and w2 <= BITS_MAX2:
        return "bits1" if w2 <= BITS_MAX1 else "bits2"
    per = -(-w2 // 64)
    if _chunk(w2) >= 16:
        for n in (8, 16, 32):
            if per <= n:
                return "wave%d" % n
    return "full"


RESOLVER_WIDTHS = [512, 513, 1024, 1025, 1984, 1985, 2048, 2049, 3968, 3969, 4100]
RESOLVER_S = [1.7, -0.5, INF, 0.9, 0.0]


@pytest.mark.parametrize("w", RESOLVER_WIDTHS)
def test_right_view_resolvers_at_chunk_seams(wslib, gpu_ctx, w):
    """Heights of one chunk, one either side and three chunks and a bit: the chunk hand-off of the wave resolvers
    (rows chunk - 1 | chunk, 2 chunk - 1 | 2 chunk ...) with the map changed by the factor on both sides."""
    chunk = _chunk(w)
    c = chunk if chunk >= 16 else 16
    expect = {"wave8": (1, 512), "wave16": (513, 1024), "wave32": (1025, 2048), "full": (2049, 1 << 30)}
    for s in RESOLVER_S:
        r = _resolver(w, s)
        if r in expect:
            assert expect[r][0] <= w <= expect[r][1], (w, s, r)
        else:
            assert (r == "bits1") == (w <= 1984), (w, s, r)
        for h in (c - 1, c, c + 1, 3 * c + 5):
            seams = [k * c + d for k in range(1, h // c + 1) for d in (-1, 0) if k * c < h] if r.startswith("wave") else []
            _check(wslib, gpu_ctx, "right", (w, h, 48, w + h), 7, 0, 48, s, rows=seams, what=(w, h, s, r, chunk))


FULL_HEIGHT = [(512, 1988, 1.7, "wave8"), (1024, 1988, -0.5, "wave16"), (2048, 1988, INF, "wave32"),
               (4096, 2160, 1.7, "full"), (1984, 1988, 0.9, "bits1"), (3968, 1988, 0.0, "bits2"), (4100, 994, 0.9, "full")]


@pytest.mark.parametrize("w,h,s,resolver", FULL_HEIGHT)
def test_right_view_resolver_at_full_height(wslib, gpu_ctx, w, h, s, resolver):
    assert _resolver(w, s) == resolver
    _check(wslib, gpu_ctx, "right", (w, h, 64, 3 * w + h), 7, 0, 64, s, what=(w, h, s, resolver))
    assert "march" in gpu_ctx.last_launch()["kernel"]


LINEAR = [(512, 994, 1.7, 200, "wave8"), (1000, 994, -0.5, 200, "wave16"), (2000, 994, INF, 200, "wave32"),
          (2964, 994, 1.7, 200, "full"), (1482, 994, 0.9, 200, "bits1"), (2964, 994, 0.9, 200, "bits2"),
          (4200, 24, 0.9, 4100, "full"), (4200, 24, 1.7, 4100, "full")]


@pytest.mark.parametrize("w,h,s,rng,resolver", LINEAR)
def test_linear_search_per_resolver(wslib, gpu_ctx, w, h, s, rng, resolver):
    """LinearSearch (1 x 1 SSD, ws_linear_kernel; ranges above 4096 ws_generic_kernel) through the generic prepare and
    each resolver."""
    assert _resolver(w, s) == resolver
    _check(wslib, gpu_ctx, "linear", (w, h, 200, w + 5 * h), 1, 0, rng, s, what=(w, h, s, rng, resolver))
    # (launch_linear hands ranges above kLinearMaxRange = 4096 to the brute-force kernel)
    assert gpu_ctx.last_launch()["kernel"] == ("ws_linear_kernel" if rng <= 4096 else "ws_generic_kernel")


# ---- right-view prepare (box + ring on the planes, or generic) -------------------------------------------------------
def _centred(ww, nd):
    """ssd_needs_centring (ws_device.h), with the key bound test_seam_sweep holds it to."""
    c = 2 * ww * ww * 3 * 255 * 255 * nd >= 1 << 28
    if c:
        assert (255 * 255 - 127 * 127) * ww * ww * 3 * nd < 1 << 28
    return c


@pytest.mark.parametrize("name", ["config2", "config3"])
def test_right_view_prepare_at_config_shapes(wslib, gpu_ctx, name):
    """Plain SSD (config 2) and SAD through the halo cost twin (config 3), s = 0.9."""
    w, h, bs, cost, maxd, seed = WORKLOADS[name]
    _check(wslib, gpu_ctx, "right", (w, h, maxd, seed), bs, 0, maxd, 0.9, cost)
    kernel = gpu_ctx.last_launch()["kernel"]
    assert "march" in kernel and (("halo" in kernel) == (name == "config3")), kernel


@pytest.mark.parametrize("bs", [13, 19])
def test_right_view_prepare_centred_and_generic_at_full_size(wslib, gpu_ctx, bs):
    """bs 13 (12 x 12 windows): a centred SSD window other than the pipeline's 16 x 16; bs 19: no marching kernel,
    the generic prepare."""
    w, h, maxd = 1482, 994, 200
    p = _plan(wslib, "right", bs, "ssd", maxd, w, h, mind=SMOOTH_RIGHT_MIND)
    if bs == 13:
        assert p["marching"] and _centred(bs - 1, p["d_per_thread"]), p
    else:
        assert not p["marching"], p
    _check(wslib, gpu_ctx, "right", (w, h, maxd, bs), bs, 0, maxd, 0.9)
    assert ("march" in gpu_ctx.last_launch()["kernel"]) == (bs == 13)


BOX_FORMS = [(7, "ssd"), (7, "sad"), (17, "ssd")]          # plain SSD, SAD, centred SSD (16 x 16, 4 per thread)


def _find_box_seam(wslib, bs, cost, seam):
    """A right-view shape whose marching interior (the box kernel's 64 x kBoxRows tiles) has a partial last tile of
    `seam` columns or rows: width = 1 or 63 (mod 64), height = 1 or 15 (mod 16)."""
    axis, want = seam.split("_")
    want = int(want)
    if axis == "w":
        scan = [(w, 60) for w in range(200, 400)]
    else:
        scan = [(300, h) for h in range(60, 120)]
    for w, h in scan:
        p = _plan(wslib, "right", bs, cost, 64, w, h, mind=SMOOTH_RIGHT_MIND)
        iw, ih = p["interior_x1"] - p["interior_x0"], p["interior_y1"] - p["interior_y0"]
        if p["marching"] and (iw % 64 == want if axis == "w" else ih % 16 == want):
            return w, h, p
    pytest.fail("no shape with %s" % seam)


@pytest.mark.parametrize("seam", ["w_1", "w_63", "h_1", "h_15"])
@pytest.mark.parametrize("bs,cost", BOX_FORMS)
def test_right_view_prepare_box_tile_seams(wslib, gpu_ctx, bs, cost, seam):
    """The box kernel tiles the right view's interior in canonical (mirrored) columns, x = ox0 + 64 k with original
    column wa - 1 - x (ws_smooth_prepare_box_kernel), and rows downwards from oy0: the partial last tile holds the
    original columns [interior_x0, interior_x0 + r) and the rows [interior_y1 - r, interior_y1).  The factor has to
    change the map on both sides of that seam: a black column just left of the seam's two columns (a zero run beside
    them) and tie texture from column 0 on."""
    w, h, p = _find_box_seam(wslib, bs, cost, seam)
    assert (cost == "ssd" and bs == 17) == (cost == "ssd" and _centred(bs - 1, p["d_per_thread"])), p
    r = int(seam.split("_")[1])
    x0, y1 = p["interior_x0"], p["interior_y1"]
    key = (w, h, 64, w * h, None, None, 7, x0 + r - 2)
    # (beside the black column d = 0 wins outright -- the column is in both images -- so it takes s = inf, which
    # refuses d = 0 beside a zero, to change the first interior columns)
    _check(wslib, gpu_ctx, "right", key, bs, 0, 64, INF if seam[0] == "w" else 0.9, cost,
           rows=[y1 - r - 1, y1 - r] if seam[0] == "h" else (), cols=[x0 + r - 1, x0 + r] if seam[0] == "w" else (),
           what=(bs, cost, seam, w, h, p))


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_right_view_prepare_after_multi_pass_d(wslib, gpu_ctx, cost):
    """D past one d-group pass: the cost plane is written in the last pass (ws_march_kernel.h)."""
    w, h = 1700, 100
    maxd = next(d for d in range(400, 1600, 8)
                if _plan(wslib, "right", 7, cost, d, w, h, mind=SMOOTH_RIGHT_MIND)["passes"] >= 2)
    _check(wslib, gpu_ctx, "right", (w, h, maxd, 17), 7, 0, maxd, 0.9, cost, what=(cost, maxd))


def test_min_disparity_above_zero_with_a_factor(wslib, gpu_ctx):
    """Right view: with min_disparity > 0, d = 0 is no candidate and the factor can never act (same map as s = 1);
    left view: the reference never reads min_disparity (BlockSearch.cpp:53)."""
    key = (600, 150, 64, 41)
    for s in (0.9, 1.7):
        want = _ref("right", key, 7, 5, 64, s, "ssd")
        assert np.array_equal(want, _ref("right", key, 7, 5, 64, 1.0, "ssd"))
        _assert_same(_run(wslib, gpu_ctx, "right", key, 7, 5, 64, s), want, ("right", s))
        _check(wslib, gpu_ctx, "left", key, 7, 5, 64, s)


def test_unequal_pair_both_views(wslib, gpu_ctx):
    """The MotorcycleE shape (1481 x 1038 against 1495 x 1052): the left view, and with the roles swapped (the right
    view needs the wider image on the left) both views."""
    for key, views in (((1481, 1038, 140, 31, 1495, 1052), ("left",)), ((1495, 1052, 140, 31, 1481, 1038), ("left", "right"))):
        for view in views:
            for s in (0.9, 1.7):
                _check(wslib, gpu_ctx, view, key, 7, 0, 140, s)


# ---- left view (launch_smooth_left) ---------------------------------------------------------------------------------
BAND_ROWS, BAND_FILL, TOP_SLAB = 32, 5, 8                  # kBandRows, kBandFill, kTopSlab (ws_smooth.hip)
LDS_PLANES, LDS_TW = 152 * 1024, 158 * 1024                # the limits launch_smooth_left holds lds / lds_t to
COMPILED_BS = (5, 7, 9, 17)                                # WS_LEFT_BS: the block sizes with a compile-time form


def _left_lds(bs, maxd):
    """launch_smooth_left's LDS bytes: the planes' moving windows, and with their row-major copies (TW)."""
    half = (bs - 1) // 2
    rp = BAND_ROWS + 2 * half + 2
    cwa = 2 * half + BAND_ROWS + 34 + BAND_FILL
    cwb = maxd + cwa
    cwa_t = 2 * half + BAND_ROWS + 6 + BAND_FILL
    cwb_t = maxd + cwa_t
    lds = (cwa + cwb) * rp * 4
    lds_t = (cwa_t + cwb_t) * rp * 4 + (((cwa_t + bs + 1) & ~1) + ((cwb_t + bs + 1) & ~1)) * (rp - 1) * 4
    return lds, lds_t


def _left_limit(bs, which):
    """The largest D whose planes form (which = 0) / TW form (1) still fits."""
    cap = (LDS_PLANES, LDS_TW)[which]
    d = 1
    while _left_lds(bs, d + 1)[which] <= cap:
        d += 1
    return d


def _left_form(wslib, bs, cost, maxd, w, h, s):
    """(MODE, BS, TW) of the ws_smooth_left_bands_kernel this call launches."""
    p = _plan(wslib, "left", bs, cost, maxd, w, h)
    lds, lds_t = _left_lds(bs, maxd)
    if not p["marching"] or lds > LDS_PLANES:
        return (-1, 0, False)
    mode = 0 if cost == "sad" else (2 if _centred(bs, p["d_per_thread"]) else 1)
    form_bs = bs if bs in COMPILED_BS else 0
    tw = form_bs != 0 and s < 1.0 and lds_t <= LDS_TW
    return (mode, form_bs, tw)


@pytest.mark.parametrize("s", [0.9, -0.5])
def test_left_view_config3_whole_map(wslib, gpu_ctx, s):
    w, h, bs, cost, maxd, seed = WORKLOADS["config3"]
    assert _left_form(wslib, bs, cost, maxd, w, h, s) == (0, 9, False)
    _check(wslib, gpu_ctx, "left", (w, h, maxd, seed), bs, 0, maxd, s, cost)


def test_left_view_config5_whole_map(wslib, gpu_ctx):
    """D = 1024 is past the planes form's LDS limit: the global-memory form."""
    w, h, bs, cost, maxd, seed = WORKLOADS["config5"]
    assert _left_form(wslib, bs, cost, maxd, w, h, 0.9) == (-1, 0, False)
    _check(wslib, gpu_ctx, "left", (w, h, maxd, seed), bs, 0, maxd, 0.9, cost)
    gpu_ctx.device_status()


LEFT_FORM_CASES = ([(bs, cost, 64, 400, s) for bs in (5, 7, 9, 11, 17, 19) for cost in ("ssd", "sad") for s in (0.9, 1.7)]
                   + [(13, "ssd", 512, 700, 0.9), (11, "ssd", 512, 700, -0.5)])
REACHABLE = ({(0, b, t) for b in COMPILED_BS for t in (False, True)} | {(0, 0, False)}
             | {(1, b, t) for b in (5, 7, 9) for t in (False, True)} | {(1, 0, False)}
             | {(2, 17, False), (2, 17, True), (2, 0, False), (-1, 0, False)})


def test_left_view_every_band_kernel_form(wslib, gpu_ctx):
    """Every reachable (MODE, BS, TW): SAD / plain SSD / centred SSD (17 x 17 always, 11 and 13 at 8 disparities per
    thread), the compile-time block sizes and the run-time one (11, 13), with (s < 1, fits) and without the
    row-major copies, and bs 19 (no marching kernel: global memory)."""
    seen = set()
    for bs, cost, maxd, w, s in LEFT_FORM_CASES:
        h = 3 * BAND_ROWS + bs + 4
        form = _left_form(wslib, bs, cost, maxd, w, h, s)
        seen.add(form)
        _check(wslib, gpu_ctx, "left", (w, h, maxd, bs * 7 + maxd), bs, 0, maxd, s, cost, what=(bs, cost, maxd, s, form))
    gpu_ctx.device_status()
    assert seen == REACHABLE, (sorted(seen), sorted(REACHABLE))


@pytest.mark.parametrize("bs", [7, 17])
def test_left_view_d_either_side_of_the_lds_limits(wslib, gpu_ctx, bs):
    for which in (0, 1):
        lim = _left_limit(bs, which)
        for maxd in (lim, lim + 1):
            w, h = maxd + 140, BAND_ROWS * 2 + bs + 3
            form = _left_form(wslib, bs, "ssd", maxd, w, h, 0.9)
            if which == 0:
                assert (form[0] == -1) == (maxd > lim), (bs, maxd, form)
            else:
                assert form[2] == (maxd <= lim), (bs, maxd, form)
            _check(wslib, gpu_ctx, "left", (w, h, maxd, maxd), bs, 0, maxd, 0.9, what=(bs, which, maxd, form))
    gpu_ctx.device_status()


@pytest.mark.parametrize("s", [0.9, -0.5])
@pytest.mark.parametrize("dh", [-1, 0, 1])
def test_left_view_interior_heights_at_band_seams(wslib, gpu_ctx, dh, s):
    """Interior height 32k - 1, 32k, 32k + 1 (k = 3): the last band full, one row short, one row alone; the factor
    changes rows 32j - 1 and 32j of the interior on both sides of every band seam."""
    bs, half = 7, 3
    ih = 3 * BAND_ROWS + dh
    h = ih + 2 * half
    rows = [half + BAND_ROWS * j + d for j in range(1, 4) for d in (-1, 0) if BAND_ROWS * j + d < ih]
    _check(wslib, gpu_ctx, "left", (500, h, 64, h), bs, 0, 64, s, rows=rows)
    gpu_ctx.device_status()


def test_left_view_top3_slab_boundaries(wslib, gpu_ctx):
    """s outside [0, 1]: the top-3 table in slabs of 8 disparities counted down from min(D, w1 - 1 - 2 half): D = 8k,
    8k +- 1, and D clamped by the width to 8k, 8k + 1."""
    bs, half = 7, 3
    for s in (1.7, -0.5):
        for w, maxd in ((300, 39), (300, 40), (300, 41), (55, 200), (56, 200)):
            d_max = min(maxd, w - 1 - 2 * half)
            assert d_max in (39, 40, 41, 48, 49), d_max
            h = 2 * BAND_ROWS + 11
            _check(wslib, gpu_ctx, "left", (w, h, 64, w + maxd), bs, 0, maxd, s, what=(w, maxd, d_max, s))
    gpu_ctx.device_status()


CHILD = r"""
import sys
import numpy as np
import stereo_reconstruction_amd as ws
sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_smooth_whole_map import _scene
from oracle import oracle
w, h, bs, maxd, s = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6])
left, right = _scene(w, h, maxd, 77)
ctx = ws.WindowSearch(0)
got = ctx.search(ws.make_params(ws.VIEW_LEFT, bs, 0, maxd, s, "ssd"), left, right)
ctx.device_status()
want = oracle.fast_left(left, right, bs, 0, maxd, smooth=s)
idle = np.array_equal(want, oracle.fast_left(left, right, bs, 0, maxd))
print("RESULT", bool(np.array_equal(got, want)), "IDLE", idle)
"""


@pytest.mark.parametrize("knob,s", [("WS_LEFT_TW=0", 0.9), ("WS_TOP3_WHOLE=1", 1.7)])
def test_left_view_development_knobs_in_a_child(knob, s):
    """The knobs are read once per process: one child each, at 1482 x 994, bs 7, D 200 (the row-major copies fit
    there, so WS_LEFT_TW=0 takes the other form; WS_TOP3_WHOLE=1 the whole-window top-3 kernel)."""
    name, value = knob.split("=")
    env = dict(os.environ, PYTHONPATH=ROOT)
    env[name] = value
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, "1482", "994", "7", "200", str(s)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "RESULT True IDLE False" in r.stdout, r.stdout + r.stderr


# ---- entry points ---------------------------------------------------------------------------------------------------
def test_search_many_pipeline_call_on_training_h_shapes(wslib, gpu_ctx, oracle):
    """The reference pipeline's right-view call (bs 17, D 200, s = 0.9) through the batched host path, float64."""
    keys = [(w, h, 200, 200 + i) for i, (_n, w, h, _d) in enumerate(TRAINING_H)]
    p = wslib.make_params(wslib.VIEW_RIGHT, 17, 0, 200, 0.9, "ssd")
    many = gpu_ctx.search_many(p, [_scene(*k) for k in keys], dtype=np.float64)
    for (name, *_), key, got in zip(TRAINING_H, keys, many):
        want = _ref("right", key, 17, 0, 200, 0.9, "ssd")
        assert not np.array_equal(want, oracle.fast_right(*_scene(*key), 17, 0, 200)), name
        _assert_same(got, want, name)


def test_two_streams_alternating_views_with_growing_scratch(wslib, gpu_ctx):
    """Left view s = 0.9 and right view s = 1.7 alternating on two streams, no host synchronisation between calls,
    each pair bigger than the last (top3, sel, sel_planes, cost and the band words are reallocated)."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = []
    for i, (w, h) in enumerate([(300, 140), (520, 230), (760, 330), (1100, 470)]):
        view, s = ("left", 0.9) if i % 2 == 0 else ("right", 1.7)
        left, right = _scene(w, h, 64, 900 + i)
        tl, tr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
        out = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
        cases.append(((w, h, 64, 900 + i), view, s, tl, tr, out, streams[i % 2]))
    torch.cuda.synchronize()
    for key, view, s, tl, tr, out, st in cases:
        gpu_ctx.search_device(wslib.make_params(_view(wslib, view), 7, 0, 64, s, "ssd"), tl, tr, out, st.cuda_stream)
    for st in streams:
        gpu_ctx.device_status(st.cuda_stream)
    torch.cuda.synchronize()
    for key, view, s, tl, tr, out, st in cases:
        want = _ref(view, key, 7, 0, 64, s, "ssd")
        assert not np.array_equal(want, _ref(view, key, 7, 0, 64, 1.0, "ssd"))
        _assert_same(out.cpu().numpy().astype(np.float64), want, (key, view, s))


@pytest.mark.parametrize("view,s", [("left", 0.9), ("right", 1.7), ("right", 0.9)])
def test_host_outputs_float32_and_float64(wslib, gpu_ctx, view, s):
    key = (1200, 700, 128, 55)
    got64 = _check(wslib, gpu_ctx, view, key, 9, 0, 128, s)
    got32 = _run(wslib, gpu_ctx, view, key, 9, 0, 128, s, dtype=np.float32)
    assert got32.dtype == np.float32 and got64.dtype == np.float64
    _assert_same(got32.astype(np.float64), got64, (view, s, "f32 vs f64"))
