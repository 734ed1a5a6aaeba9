"""Semi-global matching on the device at every form ws_sgm.hip / ws_sgm.cpp can take: every count NJ of disparities a
path lane keeps in registers (1 ... 32, both ends of each upper band), both storage widths of the costs and of the
sums on either side of their switches, right images larger than the left one, and the context's shared scratch under
calls that do not wait for each other.  Every comparison is a whole map, bit for bit against tests/sgm_ref.py, with
the sub-pixel parabola unless said otherwise; every case asserts the form it ran:
  * NJ from nd, which the test restates from the call's geometry (sgm_inputs.nd_of / nj_of);
  * the 16- or 32-bit costs and 32- or 64-bit sums from ws_sgm_scratch_bytes, whose formula fixes both widths.
The register-count inputs are the staircase pairs of tests/sgm_inputs.py; tests/test_sgm_inputs.py shows on the CPU
that their maps depend on the link between the two sides of every multiple of 64."""
import functools

import numpy as np
import pytest

from sgm_inputs import GEOMETRIES, STAIRCASES, geometry_case, nd_of, nj_of, staircase_case, staircase_pair
from sgm_ref import sgm_np
from test_gpu_sgm import _torch, assert_bits, dev_image, device_map, params_of

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3


def widths_of(wslib, p, L, R, paths, p1, p2, nd):
    """(cost16, sum64) of the call, from the scratch it asks for: 4 B per pixel of candidate intervals, then nd costs
    of 2 or 4 B and nd sums of 4 or 8 B per pixel, each block rounded up to 256 B."""
    h, w = (L if p.view == wslib.VIEW_LEFT else R).shape[:2]
    vol = w * h * nd

    def up(n):
        return (n + 255) & ~255
    forms = {up(4 * w * h) + up(vol * c) + up(vol * s): (int(c == 2), int(s == 8)) for c in (2, 4) for s in (4, 8)}
    assert len(forms) == 4, "the four layouts must differ in size for the scratch to name the one chosen"
    return forms[wslib.sgm_scratch_bytes(p, L, R, paths, p1, p2)]


def check_form(wslib, ctx, L, R, view, bs, mind, maxd, cost, paths, p1, p2, nd, nj, widths, subpixel=True, pad=0):
    p = params_of(wslib, view, bs, mind, maxd, cost, subpixel)
    assert nd_of(view, bs, mind, maxd, L.shape[1]) == nd and nj_of(nd) == nj, (nd, nj)
    assert widths_of(wslib, p, L, R, paths, p1, p2, nd) == widths
    got = device_map(wslib, ctx, p, L, R, paths, p1, p2, pad=pad)
    want = sgm_np(L, R, view, bs, mind, maxd, cost, paths, p1, p2, subpixel=subpixel)
    assert_bits(got, want, (view, bs, mind, maxd, cost, paths, p1, p2, subpixel, L.shape, R.shape))
    return want


# ---- registers per lane -------------------------------------------------------------------------------------------------
NJ = {"129-left": 4, "256-right": 4, "257-left": 8, "512-right": 8, "513-right": 16, "1024-left": 16, "1025-left": 32,
      "1025-right": 32, "2048-left": 32, "2048-right": 32, "600-left-levels": 16, "600-right-levels": 16, "seams-left": 8}


@pytest.mark.parametrize("name", sorted(STAIRCASES, key=lambda n: (STAIRCASES[n][4], n)))
def test_register_counts(wslib, gpu_ctx, name):
    """Staircase pairs at the first and last nd of the bands of NJ = 8, 16 and 32 and at 129 and 256 for NJ = 4, each
    band in both views, 4 and 8 paths, 16- and 32-bit costs with 32- and 64-bit sums; few-level pairs near nd = 600
    (ties at large j: the winner's 12-bit tags); and 364 x 72 at nd = 310, across the cost kernel's strip seams (rows
    32, 64), its tile seams (every 64 columns) and the register seams of NJ = 8.  The two nd = 2048 cases take the
    CPU reference's time (about 12 s each), the others a few seconds at the most."""
    L, R, args, nd, widths = staircase_case(name)
    want = check_form(wslib, gpu_ctx, L, R, *args, nd, NJ[name], widths, pad=3 if nd % 2 else 0)
    view, mind = args[0], args[2]
    j = np.round(want[want != 0]) - (1 if view == "left" else mind)
    assert ((j >= 64 * ((nd - 1) // 64)) & (j < nd)).any(), "no winner in the top live register"
    if name == "seams-left":
        assert L.shape[0] >= 70 and L.shape[1] >= 330 and nd >= 300


def test_one_disparity_past_the_limit_is_refused(wslib, gpu_ctx):
    """nd = 2049 is WS_ERR_UNSUPPORTED in both views; 2048, and a larger max_disparity the geometry clips to 2048, are
    accepted; the context still gives the reference's map afterwards."""
    torch = _torch()
    L, R = staircase_pair(2060, 3, 1, 40, 5)
    tl, tr = dev_image(torch, L), dev_image(torch, R)
    out = torch.zeros((3, 2060), dtype=torch.float32, device="cuda")
    for view, mind, maxd in (("left", 0, 2049), ("right", 0, 2049), ("right", 7, 2056)):
        p = params_of(wslib, view, 3, mind, maxd, "sad", True)
        assert wslib.validate_sgm(p, L, R, 8, 20, 400) == UNSUPPORTED
        with pytest.raises(wslib.WsError) as e:
            gpu_ctx.search_sgm_device(p, tl, tr, out, 8, 20, 400)
        assert e.value.code == UNSUPPORTED
    assert wslib.validate_sgm(params_of(wslib, "left", 3, 0, 2048, "sad", True), L, R, 8, 20, 400) == 0
    assert wslib.validate_sgm(params_of(wslib, "right", 3, 7, 2055, "sad", True), L, R, 8, 20, 400) == 0
    assert wslib.validate_sgm(params_of(wslib, "left", 3, 0, 5000, "sad", True), L[:, :2051], R[:, :2051], 8, 20, 400) == 0
    assert wslib.validate_sgm(params_of(wslib, "left", 3, 0, 5000, "sad", True), L[:, :2052], R[:, :2052], 8, 20, 400) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call wrote to the map"
    La, Ra, args, nd, widths = staircase_case("129-left")
    check_form(wslib, gpu_ctx, La, Ra, *args, nd, 4, widths)


# ---- storage widths -----------------------------------------------------------------------------------------------------
BIG = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def width_pair(view):
    """100 x 16, a staircase over 70 disparities (two registers per lane)."""
    return staircase_pair(100, 16, 1, 69, 31 + (view == "right"), view)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("p1", [0, 1000, BIG])
@pytest.mark.parametrize("bs", [3, 9])
def test_16_bit_costs_under_64_bit_sums(wslib, gpu_ctx, bs, p1, paths):
    """SAD up to 9 x 9 keeps its costs in 16 bits; P2 = 2^31 - 1 needs 64-bit sums: the <uint16_t, unsigned long long>
    kernels, in both views."""
    for view in ("left", "right"):
        L, R = width_pair(view)
        mind = 0 if view == "left" else 1
        maxd = 70 + mind
        check_form(wslib, gpu_ctx, L, R, view, bs, mind, maxd, "sad", paths, p1, BIG, 70, 2, (1, 1))


@pytest.mark.parametrize("view", ["left", "right"])
def test_either_side_of_the_64_bit_sum_switch(wslib, gpu_ctx, view):
    """8 paths, SAD 9 x 9 (Cmax = 3 * 255 * 81): at P2 = 536870911 - Cmax, 8 (Cmax + P2) = 2^32 - 8 still fits 32-bit
    sums; one more does not."""
    cmax = 3 * 255 * 81
    L, R = width_pair(view)
    mind = 0 if view == "left" else 1
    for p1 in (1000, None):
        for p2, sum64 in ((536870911 - cmax, 0), (536870912 - cmax, 1)):
            assert (8 * (cmax + p2) > 2 ** 32 - 1) == bool(sum64)
            check_form(wslib, gpu_ctx, L, R, view, 9, mind, 70 + mind, "sad", 8, p2 if p1 is None else p1, p2, 70, 2,
                       (1, sum64))


def saturated_pair(w=96, h=44, cell=16):
    """An all-255 left image and a right image of 16 x 16 cells of 1 and 255: windows inside a cell of 1 cost 3 * 254
    per pixel: 61 722 for 9 x 9 SAD in the left view (16 bits hold it, through (CT)acc) and 92 202 for 11 x 11 (they
    would not); the right view's windows are one row and one column smaller, 48 768 and 76 200."""
    L = np.full((h, w, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    R = np.where(((yy // cell + xx // cell) % 2 == 0)[..., None], 1, 255).astype(np.uint8)
    return L, np.ascontiguousarray(np.broadcast_to(R, (h, w, 3)))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("bs,cost16", [(9, 1), (11, 0)])
def test_either_side_of_the_16_bit_cost_switch(wslib, gpu_ctx, view, bs, cost16):
    from sgm_ref import volume
    L, R = saturated_pair()
    peak = 3 * 254 * (bs * bs if view == "left" else (bs - 1) * (bs - 1))
    assert (peak <= 0xffff) == bool(cost16) and (bs, view, peak) in ((9, "left", 61722), (11, "left", 92202), (9, "right", 48768), (11, "right", 76200))
    assert int(volume(L, R, view, bs, 0, 30, "sad")[0].max()) == peak
    nd = nd_of(view, bs, 0, 30, L.shape[1])
    for paths, p1, p2 in ((8, 500, 5000), (4, 0, 70000)):
        check_form(wslib, gpu_ctx, L, R, view, bs, 0, 30, "sad", paths, p1, p2, nd, 1, (cost16, 0))


# ---- geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_larger_right_images(wslib, gpu_ctx, name):
    """The right image wider than the left one, taller, or both; in the right view wider by more than max_disparity
    (whole columns without a candidate hold -x) and one row taller, with min_disparity 0 and above."""
    maxd = 70
    L, R, view, mind = geometry_case(name, 150, 34, maxd)
    i = sorted(GEOMETRIES).index(name)
    bs, cost = ((5, "sad"), (7, "ssd"), (3, "ssd"), (9, "sad"))[i % 4]
    paths, p1, p2 = ((8, 60, 700), (4, 900, 20000), (8, 300, 9000), (4, 100, 1500))[i % 4]
    nd = nd_of(view, bs, mind, maxd, L.shape[1])
    want = check_form(wslib, gpu_ctx, L, R, view, bs, mind, maxd, cost, paths, p1, p2, nd, nj_of(nd),
                      (int(cost == "sad"), 0), pad=i % 2)
    assert nd > 64
    if view == "right" and GEOMETRIES[name][1] is None:
        xs = np.arange(L.shape[1], R.shape[1])
        assert len(xs) > maxd and (want[:L.shape[0], L.shape[1]:] == -xs[None, :]).all()
    if R.shape[0] > L.shape[0] and view == "right":
        assert (want[L.shape[0]:] == 0).all()


# ---- the shared scratch -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_call():
    """640 x 120, nd 128, 4 paths: long enough on the device (640-step path lines, about ten launches) that the call
    enqueued right after it finds it running.  That is an assumption about timing, not something these tests can
    prove: if it does not hold they still compare every map, but no longer exercise the wait."""
    from test_subpixel_reference import shifted_pair
    L, R = shifted_pair(640, 120, 37, 5)
    args = ("left", 3, 0, 128, "sad", 4, 200, 1600)
    return L, R, args, sgm_np(L, R, *args, subpixel=True)


@functools.lru_cache(maxsize=None)
def other_calls():
    from test_subpixel_reference import shifted_pair
    L, R = shifted_pair(200, 40, 21, 6)
    right = ("right", 5, 2, 90, "ssd", 8, 500, BIG)          # 32-bit costs, 64-bit sums: another layout in the block
    left = ("left", 5, 0, 60, "sad", 8, 50, 400)
    return L, R, right, sgm_np(L, R, *right, subpixel=True), left, sgm_np(L, R, *left, subpixel=True)


def enqueue(wslib, ctx, keep, L, R, args, stream):
    torch = _torch()
    view, bs, mind, maxd, cost, paths, p1, p2 = args
    p = params_of(wslib, view, bs, mind, maxd, cost, True)
    h, w = (L if view == "left" else R).shape[:2]
    out = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    keep.append(out)
    return p, out, lambda tl, tr: ctx.search_sgm_device(p, tl, tr, out, paths, p1, p2, stream=stream.cuda_stream)


def test_two_streams_share_the_scratch_without_a_host_wait(wslib):
    """Stream A, at once a different search on stream B, then A again, on one context, the host waiting only at the
    end: B's kernels must wait for A's (the lease of the SGM scratch), A's second call for B's."""
    torch = _torch()
    La, Ra, a_args, a_want = long_call()
    Lb, Rb, b_args, b_want, c_args, c_want = other_calls()
    ctx = wslib.WindowSearch(0)
    try:
        ta, tb = (dev_image(torch, La), dev_image(torch, Ra)), (dev_image(torch, Lb), dev_image(torch, Rb))
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        keep = []
        calls = [enqueue(wslib, ctx, keep, La, Ra, a_args, sa) + (ta,), enqueue(wslib, ctx, keep, Lb, Rb, b_args, sb) + (tb,),
                 enqueue(wslib, ctx, keep, Lb, Rb, c_args, sa) + (tb,), enqueue(wslib, ctx, keep, La, Ra, a_args, sb) + (ta,)]
        torch.cuda.synchronize()                 # the images and the NaN maps are in place; from here on no host wait
        for _, _, call, imgs in calls:
            call(*imgs)
        torch.cuda.synchronize()
        for (_, out, _, _), want, what in zip(calls, (a_want, b_want, c_want, a_want), ("A", "B", "A again", "B again")):
            assert_bits(out.cpu().numpy(), want, what)
    finally:
        ctx.close()


def test_the_scratch_grows_under_calls_in_flight(wslib):
    """A fresh context: a call, then one that needs more scratch (sgm_ensure frees the block the first may still be
    using and allocates a larger one), then the first again, on one stream and then across two, the host waiting only
    at the end."""
    torch = _torch()
    La, Ra, a_args, a_want = long_call()
    Lb, Rb, b_args, b_want, c_args, c_want = other_calls()
    pa = params_of(wslib, a_args[0], *a_args[1:5], True)
    pc = params_of(wslib, c_args[0], *c_args[1:5], True)
    small, large = wslib.sgm_scratch_bytes(pc, Lb, Rb, *c_args[5:]), wslib.sgm_scratch_bytes(pa, La, Ra, *a_args[5:])
    assert small < large
    ta, tb = (dev_image(torch, La), dev_image(torch, Ra)), (dev_image(torch, Lb), dev_image(torch, Rb))
    for two in (False, True):
        ctx = wslib.WindowSearch(0)
        try:
            sa = torch.cuda.Stream()
            sb = torch.cuda.Stream() if two else sa
            keep = []
            calls = [enqueue(wslib, ctx, keep, Lb, Rb, c_args, sa) + (tb,), enqueue(wslib, ctx, keep, La, Ra, a_args, sb) + (ta,),
                     enqueue(wslib, ctx, keep, Lb, Rb, c_args, sa) + (tb,), enqueue(wslib, ctx, keep, Lb, Rb, b_args, sb) + (tb,)]
            torch.cuda.synchronize()
            for _, _, call, imgs in calls:
                call(*imgs)
            torch.cuda.synchronize()
            for (_, out, _, _), want, what in zip(calls, (c_want, a_want, c_want, b_want), ("small", "large", "small again", "last")):
                assert_bits(out.cpu().numpy(), want, (what, two))
        finally:
            ctx.close()
