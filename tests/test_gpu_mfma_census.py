"""The matrix-core SSD kernel (`ws_march_kernel<ssd,7x7,mfma>`, csrc/ws_march_mfma.h) at every candidate, every range
and under every caller, and the stencil kernel (`ws_march_kernel<ssd,7x7>`) on the same searches.  Whole maps,
np.array_equal against oracle.fast_left / fast_right or a closed form, no tolerance; the only sub-pixel comparison is
against the references' subpixel="float32" mode.  Every case asserts the kernel that ran (WindowSearch.last_launch),
but two: search_lr, whose last launch is the right view's, asserts the left search's kernel through ws_plan and a plain
left search on the same context, with no tuning or knob set; BatchSearch, whose contexts are its own and expose no last
launch, only INFERS it from ws_plan of every item it runs (its search_many half does assert it).

  1. census and ties: tests/mfma_inputs.py's disparity_ladder (every (d, tile column) wins: every live accumulator
     register of every lane of every wave) and tie_ladder (only the tie rules decide), on both kernels in one process;
     the ladder also at D = 100 and 255, where the poisoned triangle cuts through the tiles;
  2. every max_disparity 1 .. 256 on the smallest shape the selection rule gives the matrix kernel, and 257 (stencil);
  3. the selection rule's edges: interior widths 383 / 384, interior heights 191 / 192;
  4. a right image narrower or shorter than the left one: the validity bound b_hi, the "no valid candidate" fallback
     (value x), the zero rows below min(h1, h2), the black-pixel rule inside the fallback region;
  5. what runs on the matrix kernel's map: sub-pixel refine, the left view's smoothFactor pass, the left-right check,
     the unrectified one-call search, search_many, BatchSearch, graph capture, two contexts on two streams -- and the
     sub-pixel and smoothFactor cases again on the stencil kernel;
  6. the plan cache under alternating tunings.

tests/test_mfma_inputs.py shows on the CPU that the generated pairs meet the conditions relied on here.
"""
import os

import numpy as np
import pytest

import mfma_inputs as mi
import rectify_ref as rr
from lr_ref import lr_check
from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

BS = 7
MFMA = "ws_march_kernel<ssd,7x7,mfma>"
STENCIL = "ws_march_kernel<ssd,7x7>"
KNOBS = ("WS_MARCH_MFMA", "WS_PLAN_SLOTS", "WS_PLAN_THREADS", "WS_MAX_CHUNKS", "WS_MARCH_ND")
LADDER = (520, 8)            # width, band: 2048 rows
CONSUMER_SHAPES = [(700, 300, 100), (1500, 1000, 256)]


def _params(wslib, maxd, smooth=1.0, subpixel=False):
    return wslib.make_params(wslib.VIEW_LEFT, BS, 0, maxd, smooth, "ssd", subpixel=subpixel)


def _plan(wslib, maxd, left_shape, right_shape=None):
    return wslib.plan(_params(wslib, maxd), left_shape, right_shape or left_shape)


def _assert_same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s)"
                             % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _want(oracle, left, right, maxd, **kw):
    return oracle.fast_left(left, right, BS, 0, maxd, cost="ssd", **kw)


def _ran(ctx, kernel, what=""):
    """The last search's marching kernel, by its exact name."""
    name = ctx.last_launch()["kernel"]
    assert name == kernel, (what, kernel, ctx.last_launch())
    return name


def _search(wslib, ctx, left, right, maxd, kernel, what, want):
    got = ctx.search(_params(wslib, maxd), left, right)
    _ran(ctx, kernel, what)
    _assert_same(got, want, what)
    return got


# The stencil kernel has three instantiations for this window and which one its planner takes depends on the search's
# size and range (a host call of a megapixel and more is searched in two row bands: the shape that counts is a band's).
# ws_plan takes no tuning, so the form cannot be asked of it: it is fixed per case, as observed on an MI355X with 256
# compute units: (width, height, max_disparity) -> the kernel's name.  A retune of the stencil planner that moves a case
# to another instantiation has to update this table; the maps must stay exact either way.
STENCIL_ND4 = "ws_march_kernel<ssd,7x7,nd4>"
STENCIL_FORM = {
    (520, 2048, 256): STENCIL_ND4, (520, 2048, 100): STENCIL_ND4, (520, 2048, 255): STENCIL_ND4,
    (640, 204, 256): STENCIL_ND4, (700, 300, 100): STENCIL_ND4, (1500, 1000, 256): STENCIL,
    (390, 198, 257): STENCIL, (389, 230, 256): STENCIL_ND4, (500, 197, 256): STENCIL_ND4,
}


def _stencil(left, maxd):
    key = (left.shape[1], left.shape[0], maxd)
    assert key in STENCIL_FORM, ("no stencil instantiation recorded for this case", key)
    return STENCIL_FORM[key]


class _tuned:
    """set_tuning(threads=512) -- a forced tuning means the stencil kernel -- restored on the way out."""

    def __init__(self, ctx, on, left, maxd):
        self.ctx, self.on, self.name = ctx, on, _stencil(left, maxd) if on else MFMA

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning(threads=512)
        return self.name

    def __exit__(self, *exc):
        self.ctx.set_tuning()


def _no_knobs():
    assert not [k for k in KNOBS if k in os.environ], "a development knob is set: the selection rule is not the one tested"


# ---- 1. census and ties ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ladder():
    w, band = LADDER
    return mi.disparity_ladder(w, band, 11, range(1, 257))


@pytest.mark.parametrize("maxd", [256, 100, 255])
@pytest.mark.parametrize("kernel", ["mfma", "stencil"])
def test_census(wslib, gpu_ctx, oracle, ladder, kernel, maxd):
    _no_knobs()
    w, band = LADDER
    left, right = ladder
    want = _want(oracle, left, right, maxd)
    assert int(mi.census(want, maxd).sum()) == 128 * maxd        # every (d, tile column) is a winner of the reference
    for y, x0, d in mi.ladder_expected(w, band, range(1, 257), maxd):
        assert (want[y, x0:w - 3] == d).all(), (y, d)
    assert _plan(wslib, maxd, left.shape)["kernel_kind"] == 1
    with _tuned(gpu_ctx, kernel == "stencil", left, maxd) as name:
        got = _search(wslib, gpu_ctx, left, right, maxd, name, ("census", kernel, maxd), want)
    assert int(mi.census(got, maxd).sum()) == 128 * maxd


@pytest.mark.parametrize("kernel", ["mfma", "stencil"])
def test_ties(wslib, gpu_ctx, oracle, kernel):
    _no_knobs()
    w, band, maxd = 640, 12, 256
    left, right = mi.tie_ladder(w, band, mi.TIE_PERIODS, 5)
    assert _plan(wslib, maxd, left.shape)["kernel_kind"] == 1
    want = _want(oracle, left, right, maxd)
    with _tuned(gpu_ctx, kernel == "stencil", left, maxd) as name:
        got = _search(wslib, gpu_ctx, left, right, maxd, name, ("ties", kernel), want)
    for k, p in enumerate(mi.TIE_PERIODS):                        # the closed form, on the device's map
        x0, row = mi.tie_expected_row(w, p, maxd)
        for y in mi.clean_rows(band, k):
            assert np.array_equal(got[y, x0:w - 3], row), (kernel, p, y)


# ---- 2. every range --------------------------------------------------------------------------------------------------

def _smallest_mfma_shape(wslib):
    """The narrowest search ws_plan gives the matrix kernel, and the shortest one of that width."""
    for w in range(300, 700):
        if _plan(wslib, 256, (400, w, 3))["kernel_kind"] == 1:
            for h in range(100, 401):
                if _plan(wslib, 256, (h, w, 3))["kernel_kind"] == 1:
                    return w, h
    pytest.fail("no search narrower than 700 columns selects the matrix kernel")


def test_every_max_disparity(wslib, gpu_ctx, oracle):
    """max_disparity 1 .. 256 on one pair: the per-wave `active` mask changes at every dcount = 32 k + 2, where a tile
    holds a single live candidate; below 98 candidates the first d-wave has no live tile at all and the merge
    takes everything from LDS.  257 candidates are one too many: the stencil kernel, the same pair, still exact."""
    _no_knobs()
    w, h = _smallest_mfma_shape(wslib)
    assert (w, h) == (390, 198), (w, h)                          # interior 384 x 192: the selection rule's threshold
    left, right = mi.range_sweep_pair(w, h)
    bad = []
    for maxd in range(1, 257):
        assert _plan(wslib, maxd, left.shape)["kernel_kind"] == 1, maxd
        got = gpu_ctx.search(_params(wslib, maxd), left, right)
        _ran(gpu_ctx, MFMA, maxd)
        want = _want(oracle, left, right, maxd)
        if not np.array_equal(got, want):
            bad.append((maxd, int((got != want).sum()), np.argwhere(got != want)[0].tolist()))
    assert not bad, ("max_disparity, pixels that differ, the first one", bad[:20], len(bad))
    assert _plan(wslib, 257, left.shape)["kernel_kind"] == 0
    _search(wslib, gpu_ctx, left, right, 257, _stencil(left, 257), ("maxd", 257), _want(oracle, left, right, 257))


# ---- 3. the selection rule's edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(383 + 6, 230, False), (384 + 6, 230, True), (500, 191 + 6, False), (500, 192 + 6, True)],
                         ids=["cols383", "cols384", "rows191", "rows192"])
def test_selection_rule_edges(wslib, gpu_ctx, oracle, shape):
    _no_knobs()
    w, h, mfma = shape
    p = _plan(wslib, 256, (h, w, 3))
    assert (p["interior_x1"] - p["interior_x0"], p["interior_y1"] - p["interior_y0"]) == (w - 6, h - 6)
    assert p["kernel_kind"] == int(mfma), p
    left, right, _ = make_pair(w, h, 256, 300 + w + h)
    left[h // 2, w // 3:w // 3 + 5] = 0
    _search(wslib, gpu_ctx, left, right, 256, MFMA if mfma else _stencil(left, 256), shape, _want(oracle, left, right, 256))


# ---- 4. a narrower or shorter right image ----------------------------------------------------------------------------

def _narrowest_right(wslib, w1, h1, maxd):
    for w2 in range(1, 20):
        if wslib.validate(_params(wslib, maxd), (h1, w1, 3), (h1, w2, 3)) == 0:
            return w2
    pytest.fail("validate accepts no right image narrower than 20 columns")


SMALLER_RIGHT = [(900, 400, 500, 400, 100, 118200), (900, 400, 640, 230, 256, 896), (700, 600, 7, 600, 64, 373626),
                 (700, 400, None, 400, 64, None)]


@pytest.mark.parametrize("case", SMALLER_RIGHT, ids=["narrower", "narrower_shorter", "one_valid_centre", "narrowest"])
def test_smaller_right_image(wslib, gpu_ctx, oracle, case):
    """x - d <= b_hi = w2 - 4 cuts candidates off on the right: for x > w2 - 4 + D no candidate is valid and the map
    holds x; below min(h1, h2) - 3 it holds zeros.  Black pixels inside the fallback region stay 0."""
    import torch
    _no_knobs()
    w1, h1, w2, h2, maxd, n_fallback = case
    if w2 is None:
        w2 = _narrowest_right(wslib, w1, h1, maxd)
    left, right, _ = make_pair(w1, h1, maxd, 500 + w2, right_width=w2, right_height=h2)
    assert right.shape == (h2, w2, 3)
    hh = min(h1, h2)
    # a target centre is valid in [3, w2 - 4]: the first column without a valid candidate
    x0 = w2 - 4 + maxd + 1 if w2 >= 7 else 3
    assert 3 <= x0 < w1 - 3
    for y, x in ((hh // 2, x0), (3, w1 - 4), (hh - 8, (x0 + w1 - 4) // 2)):   # five black pixels each, inside the region
        left[y:y + 5, x] = 0
    want = _want(oracle, left, right, maxd)
    # the reference's own map shows that the case reaches what it is meant to reach
    black = (left == 0).all(axis=2)
    cols = np.broadcast_to(np.arange(w1, dtype=np.float64), (h1, w1))
    region = np.zeros((h1, w1), bool)
    region[3:hh - 3, x0:w1 - 3] = True
    assert np.array_equal(want[region & ~black], cols[region & ~black])
    assert (want[region & black] == 0).all() and int((region & black).sum()) == 15
    assert (want[hh - 3:] == 0).all()
    if n_fallback is not None:
        assert int(region.sum()) == n_fallback
    p = wslib.plan(_params(wslib, maxd), left.shape, right.shape)
    assert p["kernel_kind"] == 1, p
    got = _search(wslib, gpu_ctx, left, right, maxd, MFMA, ("host", case), want)
    assert (got[region & black] == 0).all()
    out = torch.full((h1, w1), -7.0, dtype=torch.float32, device="cuda")
    gpu_ctx.search_device(_params(wslib, maxd), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), out, None)
    torch.cuda.synchronize()
    _ran(gpu_ctx, MFMA)
    _assert_same(out.cpu().numpy().astype(np.float64), want, ("search_device", case))


# ---- 5. what runs on the matrix kernel's map -------------------------------------------------------------------------

@pytest.fixture(scope="module", params=CONSUMER_SHAPES, ids=lambda s: "%dx%d-D%d" % s)
def scene(request, wslib):
    w, h, maxd = request.param
    left, right, _ = make_pair(w, h, maxd, 70 + maxd)
    left[h // 2, w // 3:w // 3 + 5] = 0
    right[h // 3, w // 2:w // 2 + 5] = 0
    p = _plan(wslib, maxd, left.shape)
    assert p["kernel_kind"] == 1 and p["tiles"] >= 2 and p["strips"] >= 2, p
    return left, right, maxd, p


def _check_subpixel(wslib, ctx, oracle, scene, kernel):
    left, right, maxd, p = scene
    got = ctx.search(_params(wslib, maxd, subpixel=True), left, right, dtype=np.float32).astype(np.float64)
    _ran(ctx, kernel)
    _assert_same(got, _want(oracle, left, right, maxd, subpixel="float32"), ("subpixel", kernel))
    refined = got != _want(oracle, left, right, maxd)
    assert refined.mean() > 0.3
    if kernel == MFMA:                                           # refined pixels on both sides of a tile and a strip seam
        xs = p["interior_x0"] + p["tile_cols"] * (p["tiles"] // 2)
        ys = p["interior_y0"] + p["strip_rows"] * (p["strips"] // 2)
        assert p["interior_x0"] < xs < p["interior_x1"] and p["interior_y0"] < ys < p["interior_y1"], p
        assert refined[:, xs - 1].any() and refined[:, xs].any() and refined[ys - 1].any() and refined[ys].any()


def _check_smooth(wslib, ctx, oracle, scene, kernel, smooth):
    left, right, maxd, _ = scene
    got = ctx.search(_params(wslib, maxd, smooth=smooth), left, right)
    _ran(ctx, kernel)
    want = _want(oracle, left, right, maxd, smooth=smooth)
    _assert_same(got, want, ("smooth", smooth, kernel))
    assert (want != _want(oracle, left, right, maxd)).any()     # the pass changed the map


def test_subpixel_on_the_matrix_kernel(wslib, gpu_ctx, oracle, scene):
    _no_knobs()
    _check_subpixel(wslib, gpu_ctx, oracle, scene, MFMA)


@pytest.mark.parametrize("smooth", [0.9, 1.4])
def test_left_smooth_on_the_matrix_kernel(wslib, gpu_ctx, oracle, scene, smooth):
    _no_knobs()
    _check_smooth(wslib, gpu_ctx, oracle, scene, MFMA, smooth)


def test_subpixel_and_smooth_on_the_stencil_kernel(wslib, gpu_ctx, oracle, scene):
    """The same searches under a forced tuning: the dword planes the refine and the smoothFactor pass read then have
    the stencil plan's geometry."""
    _no_knobs()
    left, _, maxd, _ = scene
    with _tuned(gpu_ctx, True, left, maxd) as name:
        _check_subpixel(wslib, gpu_ctx, oracle, scene, name)
        for smooth in (0.9, 1.4):
            _check_smooth(wslib, gpu_ctx, oracle, scene, name, smooth)


def test_left_right_check(wslib, gpu_ctx, oracle, scene):
    """search_lr runs the left search, then the right one: last_launch names the right view's kernel.  The left search's
    kernel: ws_plan, no knob, no tuning, and a plain left search on this context right before."""
    _no_knobs()
    left, right, maxd, _ = scene
    gpu_ctx.set_tuning()
    dl = _want(oracle, left, right, maxd)
    _search(wslib, gpu_ctx, left, right, maxd, MFMA, "the left search alone", dl)
    dr = oracle.fast_right(left, right, BS, 0, maxd, cost="ssd")
    for md, fill in ((1.0, False), (1.0, True)):
        want_l, want_r, want_c = lr_check(dl.astype(np.float32), dr.astype(np.float32), md, fill)
        got_l, got_r = gpu_ctx.search_lr(_params(wslib, maxd), left, right, md, fill, dtype=np.float32)
        assert "march" in gpu_ctx.last_launch()["kernel"], gpu_ctx.last_launch()
        assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32)), ("left", md, fill)
        assert np.array_equal(got_r.view(np.uint32), want_r.view(np.uint32)), ("right", md, fill)
        assert gpu_ctx.last_lr_counts() == want_c
    assert _plan(wslib, maxd, left.shape)["kernel_kind"] == 1


def test_unrectified_search(wslib, gpu_ctx, oracle, scene):
    _no_knobs()
    left, right, maxd, _ = scene
    h, w = left.shape[:2]
    eye = np.eye(3)
    got = gpu_ctx.search_unrectified(_params(wslib, maxd), left, right, eye, eye)
    _ran(gpu_ctx, MFMA)
    _assert_same(got, _want(oracle, left, right, maxd), "identity homographies")
    # one real pair of homographies: rectify (NumPy restatement) -> the reference search -> warp back with inv(H)
    H = rr.rectifying_homography(w, h, 0.8, 0.004, (1.2e-5, -0.8e-5), 1.0, (4.0, -3.0))
    Hp = rr.rectifying_homography(w, h, 0.6, -0.003, (0.9e-5, 0.5e-5), 0.985, (-2.0, 1.5))
    lw, lh = rr.rectified_size(H, w, h)
    rw, rh = rr.rectified_size(Hp, w, h)
    assert _plan(wslib, maxd, (lh, lw, 3), (rh, rw, 3))["kernel_kind"] == 1, ((lw, lh), (rw, rh))
    rl, rrt = rr.warp_linear_u8(left, H, (lh, lw)), rr.warp_linear_u8(right, Hp, (rh, rw))
    want = oracle.warp_nearest(_want(oracle, rl, rrt, maxd), rr.inv3(H), (h, w))
    got, gl, gr = gpu_ctx.search_unrectified(_params(wslib, maxd), left, right, H, Hp, rectified=True)
    _ran(gpu_ctx, MFMA)
    assert np.array_equal(gl, rl) and np.array_equal(gr, rrt)
    _assert_same(got, want, "rectifying homographies")
    assert (got != 0).mean() > 0.5


def test_search_many_and_batch_search(wslib, gpu_ctx, oracle, scene):
    """The batched host call on this context, and BatchSearch with one and two workers on one device (whole pairs and
    row bands).  BatchSearch's contexts are its own and expose no last launch: that the matrix kernel ran there is an
    inference, from ws_plan of the sub-images ws_batch.cpp hands a worker for each item (a band's rows and the window's
    halo, clipped to the image: ws_batch.cpp, "a row band"), not an observation."""
    _no_knobs()
    left, right, maxd, _ = scene
    h, w = left.shape[:2]
    l2, r2, _ = make_pair(w, h, maxd, 71 + maxd)
    pairs = [(left, right), (l2, r2), (left, right)]
    wants = [_want(oracle, l, r, maxd) for l, r in pairs[:2]]
    wants.append(wants[0])
    p = _params(wslib, maxd)
    gpu_ctx.set_tuning()
    many = gpu_ctx.search_many(p, pairs, dtype=np.float32)
    _ran(gpu_ctx, MFMA)
    for k, (got, want) in enumerate(zip(many, wants)):
        _assert_same(got.astype(np.float64), want, ("search_many", k))
    for devices, bands in (([0], False), ([0, 0], True)):
        with wslib.BatchSearch(devices) as b:
            items, banded = b.plan(p, pairs, bands=bands)
            for job, y0, y1, _ in items:                         # a band is searched with its 3 halo rows on each side
                rows = min(h, y1 + 3) - max(0, y0 - 3)
                assert _plan(wslib, maxd, (rows, w, 3))["kernel_kind"] == 1, (job, y0, y1)
            maps = b.search(p, pairs, dtype=np.float32, bands=bands)
            assert b.statuses == [0] * len(pairs)
        for k, (got, want) in enumerate(zip(maps, wants)):
            _assert_same(got.astype(np.float64), want, ("BatchSearch", devices, banded, k))


def test_graph_capture_and_replay(wslib, gpu_ctx, oracle, scene):
    """search_device captured into a graph, replayed twice on fresh inputs in the captured buffers."""
    import torch
    _no_knobs()
    left, right, maxd, _ = scene
    h, w = left.shape[:2]
    p = _params(wslib, maxd)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        gpu_ctx.search_device(p, tl, tr, out, st.cuda_stream)    # (warm-up: the scratch buffers exist)
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            gpu_ctx.search_device(p, tl, tr, out, st.cuda_stream)
    _ran(gpu_ctx, MFMA)
    for k in range(2):
        l2, r2, _ = make_pair(w, h, maxd, 900 + k)
        l2[h // 4, w // 2:w // 2 + 5] = 0
        tl.copy_(torch.from_numpy(l2))
        tr.copy_(torch.from_numpy(r2))
        out.fill_(-7.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(out.cpu().numpy().astype(np.float64), _want(oracle, l2, r2, maxd), ("replay", k))


def test_two_contexts_on_two_streams(wslib, gpu_ctx, oracle, scene):
    import torch
    _no_knobs()
    left, right, maxd, _ = scene
    h, w = left.shape[:2]
    l2, r2, _ = make_pair(w, h, maxd, 71 + maxd)
    p = _params(wslib, maxd)
    with wslib.WindowSearch(0) as other:
        jobs = []
        for ctx, (l, r) in ((gpu_ctx, (left, right)), (other, (l2, r2))):
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
                out = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
            st.synchronize()
            jobs.append((ctx, st, tl, tr, out, l, r))
        for _ in range(3):                                       # both streams busy at once, three searches each
            for ctx, st, tl, tr, out, _, _ in jobs:
                ctx.search_device(p, tl, tr, out, st.cuda_stream)
        for ctx, st, tl, tr, out, l, r in jobs:
            st.synchronize()
            _ran(ctx, MFMA)
            _assert_same(out.cpu().numpy().astype(np.float64), _want(oracle, l, r, maxd), "two contexts")


# ---- 6. the plan cache -----------------------------------------------------------------------------------------------

def test_plan_cache_under_alternating_tunings(wslib, gpu_ctx, oracle, scene):
    """One context, one shape: the cached plan must follow the tuning both ways."""
    _no_knobs()
    left, right, maxd, _ = scene
    want = _want(oracle, left, right, maxd)
    try:
        for k in range(4):
            gpu_ctx.set_tuning(threads=512)
            _search(wslib, gpu_ctx, left, right, maxd, _stencil(left, maxd), ("tuned", k), want)
            gpu_ctx.set_tuning()
            _search(wslib, gpu_ctx, left, right, maxd, MFMA, ("automatic", k), want)
    finally:
        gpu_ctx.set_tuning()
