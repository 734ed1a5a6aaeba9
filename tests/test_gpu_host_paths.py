"""How caller buffers cross at the boundary (ws_search_host / ws_enqueue_host ... ws_wait; they replace the host-only
ImageRectifier::computeDisparityMapLeft/Right, rectification.cpp:66-88, whose cv::Mat buffers are ordinary pageable
memory).  Round 2 registered the caller's buffers with the HIP runtime and one of the shapes below ended the process
(the runtime aborts on hipHostUnregister of a pointer that is not a key of its host-allocation map but lies inside
another registered range: tools/ubench/hostreg_probe.hip, profiles/r03/hostreg_probe.txt); round 3 made registration
opt-in after two GPU memory faults of unproven cause; round 4 removed it.  The library registers NO caller memory:
pageable buffers cross through its own pinned stages, memory the caller (or a framework) pinned is used as it is, a
range the runtime knows in part is staged.  Integer-valued maps cross PCIe as 16-bit integers and are widened on the
host (ws_last_wire_format).  Results must be the oracle's, bit for bit, whichever way.
"""
import ctypes

import numpy as np
import pytest

from stereo_reconstruction_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu

BS, MAXD = 7, 40
OURS = "staged"   # how a pageable buffer crosses (rounds 2-3: "registered")


def own_pages(a):
    """A copy of `a` (or an empty array of that shape / dtype) that shares no page with any other allocation: small
    numpy arrays come from the heap, where neighbours share pages and the library would (rightly) register them as
    one hull or find them inside a live range -- the tests that assert WHICH way bytes crossed need to rule that out."""
    a = np.asarray(a)
    raw = np.empty(a.nbytes + 8192, dtype=np.uint8)
    start = (-raw.ctypes.data) % 4096
    out = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def image(ws, a, width=None, height=None):
    """ws_image over a (possibly strided) uint8 array view."""
    h = a.shape[0] if height is None else height
    w = a.shape[1] if width is None else width
    return ws._Image(a.ctypes.data, w, h, a.strides[0])


def host_call(ws, ctx, p, L, R, out, out_stride=None):
    lib = ws.load_library()
    Li, Ri = image(ws, L), image(ws, R)
    code = 1 if out.dtype == np.float64 else 0
    rc = lib.ws_search_host(ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), out.ctypes.data,
                            out.shape[1] if out_stride is None else out_stride, code)
    assert rc == 0, lib.ws_last_error(ctx._h)
    return ctx.last_host_paths()


def test_pageable_numpy_buffers_cross_through_the_stages(wslib, gpu_ctx, oracle):
    left, right, _ = make_pair(300, 120, MAXD, seed=301)
    want = oracle.block_left(left, right, BS, 0, MAXD)
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD)
    out = np.empty((120, 300))
    assert host_call(wslib, gpu_ctx, p, left, right, out) == (OURS,) * 3
    assert np.array_equal(out, want)
    # the same buffers again, and fresh ones at recycled addresses with other sizes
    for h in (120, 90, 120, 60):
        l2, r2, o2 = left[:h].copy(), right[:h].copy(), np.empty((h, 300))
        assert host_call(wslib, gpu_ctx, p, l2, r2, o2) == (OURS,) * 3
        assert np.array_equal(o2, oracle.block_left(l2, r2, BS, 0, MAXD))


def test_left_and_right_cut_from_one_array(wslib, gpu_ctx, oracle):
    """Side-by-side stereo frames: both views are column ranges of ONE array, their byte spans interleave.  Round 2
    registered the first, failed on the second and copied it 'unregistered'; the runtime refuses a copy that starts
    inside a registered range and runs past its end (hipErrorInvalidValue)."""
    left, right, _ = make_pair(260, 100, MAXD, seed=302)
    frame = np.concatenate([left, right], axis=1)                    # H x 2W x 3
    L, R = frame[:, :260], frame[:, 260:]
    assert not L.flags["C_CONTIGUOUS"] and L.strides[0] == 2 * 260 * 3
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD)
    out = np.empty((100, 260), dtype=np.float32)
    assert host_call(wslib, gpu_ctx, p, L, R, out) == (OURS,) * 3
    assert np.array_equal(out.astype(np.float64), oracle.block_left(left, right, BS, 0, MAXD))
    # output rows inside the same allocation as the images (a struct-of-frames buffer)
    blob = np.zeros(frame.nbytes + 100 * 260 * 4 + 64, dtype=np.uint8)
    blob[:frame.nbytes] = frame.reshape(-1)
    f2 = blob[:frame.nbytes].reshape(frame.shape)
    o2 = blob[frame.nbytes + 64 - (blob.ctypes.data + frame.nbytes) % 64:][:100 * 260 * 4].view(np.float32).reshape(100, 260)
    assert host_call(wslib, gpu_ctx, p, f2[:, :260], f2[:, 260:], o2) == (OURS,) * 3
    assert np.array_equal(o2.astype(np.float64), oracle.block_left(left, right, BS, 0, MAXD))


def test_tiny_buffers_on_one_page(wslib, gpu_ctx, oracle):
    left, right, _ = make_pair(24, 12, 6, seed=303)
    slab = np.zeros(4096 * 3, dtype=np.uint8)
    a = slab[100:100 + left.nbytes].reshape(left.shape)
    b = slab[100 + left.nbytes + 7:100 + left.nbytes + 7 + right.nbytes].reshape(right.shape)
    a[...], b[...] = left, right
    out = slab[100 + 2 * left.nbytes + 64:]
    out = out[(-out.ctypes.data) % 8:][:12 * 24 * 8].view(np.float64).reshape(12, 24)
    p = wslib.make_params(wslib.VIEW_LEFT, 3, 0, 6, 1.0, "sad")
    assert host_call(wslib, gpu_ctx, p, a, b, out) == (OURS,) * 3
    assert np.array_equal(out, oracle.block_left(left, right, 3, 0, 6, cost="sad"))


def test_caller_pinned_memory_is_used_as_it_is(wslib, gpu_ctx, oracle):
    """Buffers the caller (here: PyTorch's pinned allocator) has pinned already are neither registered nor released by
    the library; a whole hipHostMalloc'd block cannot be registered again anyway (hipErrorInvalidValue)."""
    import torch
    left, right, _ = make_pair(300, 120, MAXD, seed=304)
    tl, tr = torch.from_numpy(left).pin_memory(), torch.from_numpy(right).pin_memory()
    to = torch.empty((120, 300), dtype=torch.float32).pin_memory()
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD)
    assert host_call(wslib, gpu_ctx, p, tl.numpy(), tr.numpy(), to.numpy()) == ("caller-pinned",) * 3
    assert np.array_equal(to.numpy().astype(np.float64), oracle.block_left(left, right, BS, 0, MAXD))
    # the blocks are still the allocator's: used and freed by their owner afterwards
    assert torch.equal(tl.cuda().cpu(), tl)
    del tl, tr, to
    torch.cuda.synchronize()


def test_crops_of_one_image_in_a_batch(wslib, gpu_ctx, oracle):
    """Crops of one image in one batch: one base pointer under two sizes (two crops with the same origin) inside the
    whole image, all alive until ws_wait -- round 2's (pointer, size) registry registered the pointer twice and
    released it twice, and the runtime aborts on the second release (profiles/r03/hostreg_probe.txt, 'twice-enclosed').
    Round 3 first registered such buffers as shared page ranges for the life of the batch; one run in ten of the whole
    suite then died in THIS test's ws_wait with a GPU memory access fault on a host heap page (a dozen registrations
    of heap memory alive while Python allocated and freed around them).  Registrations no longer outlive a call: a
    batch's pageable buffers cross through the job slots' pinned stages, whatever their layout."""
    lib = wslib.load_library()
    left, right, _ = make_pair(320, 400, MAXD, seed=307)
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD)
    crops = [(0, 400), (10, 110), (10, 210), (10, 110), (150, 400)]
    outs, keep = [], []
    for y0, y1 in crops:
        L, R = left[y0:y1], right[y0:y1]                             # contiguous row ranges: same bytes, no copy
        o = np.empty((y1 - y0, 320), dtype=np.float32)
        Li, Ri = image(wslib, L), image(wslib, R)
        keep.append((L, R, Li, Ri))
        outs.append(o)
        assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), o.ctypes.data, 320, 0) == 0
        junk = [np.empty(int(n)) for n in (3e4, 2e5, 7e3)]           # the caller's allocator at work between the calls
        del junk
    joined = np.concatenate([left, left[300:], left[:50]])          # its first 400 rows are `left` again
    o_a, o_b = np.empty((400, 320), dtype=np.float32), np.empty((100, 320), dtype=np.float32)
    Lia, Ria = image(wslib, joined[:400]), image(wslib, right)
    assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Lia), ctypes.byref(Ria), o_a.ctypes.data, 320, 0) == 0
    Ls, Rs = joined[350:450], np.concatenate([right[350:], right[300:350]])
    Lib, Rib = image(wslib, Ls), image(wslib, Rs)
    assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Lib), ctypes.byref(Rib), o_b.ctypes.data, 320, 0) == 0
    assert lib.ws_wait(gpu_ctx._h) == 0
    assert gpu_ctx.last_host_paths() == ("staged", "staged", "staged")
    for (y0, y1), o in zip(crops, outs):
        assert np.array_equal(o.astype(np.float64), oracle.block_left(left[y0:y1], right[y0:y1], BS, 0, MAXD)), (y0, y1)
    assert np.array_equal(o_a.astype(np.float64), oracle.block_left(left, right, BS, 0, MAXD))
    assert np.array_equal(o_b.astype(np.float64), oracle.block_left(np.ascontiguousarray(Ls), Rs, BS, 0, MAXD))
    # single calls on the same buffers register them for the call, and only for the call
    out = np.empty((400, 320))
    assert host_call(wslib, gpu_ctx, p, left, right, out) == (OURS,) * 3
    assert np.array_equal(out, oracle.block_left(left, right, BS, 0, MAXD))
    # pinned by the caller: direct in a batch too
    import torch
    tl, tr = torch.from_numpy(left).pin_memory(), torch.from_numpy(right).pin_memory()
    to = torch.empty((400, 320), dtype=torch.float32).pin_memory()
    Lip, Rip = image(wslib, tl.numpy()), image(wslib, tr.numpy())
    assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Lip), ctypes.byref(Rip), to.numpy().ctypes.data, 320, 0) == 0
    assert lib.ws_wait(gpu_ctx._h) == 0
    assert gpu_ctx.last_host_paths() == ("caller-pinned",) * 3
    assert np.array_equal(to.numpy().astype(np.float64), oracle.block_left(left, right, BS, 0, MAXD))


def test_staged_maps_in_a_long_batch(wslib, gpu_ctx, oracle):
    """Pageable outputs come down through the job slots' stages (as 16-bit integers, widened to doubles on the way out)
    and are handed over before a slot is used again: more pairs than slots, padded output rows."""
    lib = wslib.load_library()
    p = wslib.make_params(wslib.VIEW_RIGHT, BS, 0, MAXD, 1.0, "sad")
    pairs = [make_pair(200, 90 + 8 * i, MAXD, seed=320 + i)[:2] for i in range(5)]
    outs = [np.full((l.shape[0], 256), -7.0) for l, _ in pairs]
    keep = []
    for (l, r), o in zip(pairs, outs):
        Li, Ri = image(wslib, l), image(wslib, r)
        keep.append((Li, Ri))
        assert lib.ws_enqueue_host(gpu_ctx._h, ctypes.byref(p), ctypes.byref(Li), ctypes.byref(Ri), o.ctypes.data, 256, 1) == 0
    assert lib.ws_wait(gpu_ctx._h) == 0
    assert gpu_ctx.last_host_paths()[2] == "staged"
    for (l, r), o in zip(pairs, outs):
        assert np.array_equal(o[:, :200], oracle.block_right(l, r, BS, 0, MAXD, cost="sad")) and (o[:, 200:] == -7.0).all()


def test_an_error_in_the_middle_of_a_batch_leaves_nothing_behind(wslib, gpu_ctx, oracle):
    """search_many used to drop its buffers when a pair was refused while earlier pairs were still copying from / into
    them and their ranges stayed registered."""
    left, right, _ = make_pair(300, 120, MAXD, seed=330)
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD)
    bad = np.zeros((10, 10), dtype=np.uint8)                        # not an H x W x 3 image
    with pytest.raises(ValueError):
        gpu_ctx.search_many(p, [(left, right), (left, right), (bad, bad)])
    even = wslib.make_params(wslib.VIEW_LEFT, 6, 0, MAXD)           # the reference throws: WS_ERR_GEOMETRY
    with pytest.raises(wslib.WsError):
        gpu_ctx.search_many(even, [(left, right)])
    want = oracle.block_left(left, right, BS, 0, MAXD)
    for o in gpu_ctx.search_many(p, [(left, right)] * 3, dtype=np.float64):
        assert np.array_equal(o, want)
    out = np.empty((120, 300))
    assert host_call(wslib, gpu_ctx, p, left, right, out) == (OURS,) * 3 and np.array_equal(out, want)


def test_consumers_take_pageable_and_partly_known_buffers(wslib, gpu_ctx):
    """The Reconstruction-side calls on pageable arrays, padded rows, and a range the runtime knows IN PART (the
    caller's own pinned block with pageable bytes... cannot exist: a slice that starts inside a pinned torch block and
    is handed over as if it ran past it is not constructible safely, so the partly-known branch is driven with a view
    that ends inside the block -- known at both ends, used as it is -- and the pageable one)."""
    import torch
    rng = np.random.default_rng(9)
    disp = rng.integers(1, 60, size=(200, 300)).astype(np.float32)
    want = gpu_ctx.convert_disparity_to_depth(disp, 700.0, 0.2)
    pinned = torch.from_numpy(disp).pin_memory()
    assert np.array_equal(gpu_ctx.convert_disparity_to_depth(pinned.numpy(), 700.0, 0.2), want)
    a = gpu_ctx.remove_disparity_outliers(disp, 9, 2.0, 3.0)
    lib = wslib.load_library()
    padded = np.zeros((200, 320), dtype=np.float32)
    padded[:, :300] = disp
    assert lib.ws_remove_disparity_outliers(gpu_ctx._h, padded.ctypes.data, 300, 200, 320, 9, 2.0, 3.0) == 0
    assert np.array_equal(padded[:, :300], a) and (padded[:, 300:] == 0).all()
    pp = torch.zeros((200, 320), dtype=torch.float32).pin_memory()
    pp[:, :300] = torch.from_numpy(disp)
    assert lib.ws_remove_disparity_outliers(gpu_ctx._h, pp.numpy().ctypes.data, 300, 200, 320, 9, 2.0, 3.0) == 0
    assert np.array_equal(pp.numpy()[:, :300], a) and (pp.numpy()[:, 300:] == 0).all()


def test_integer_maps_cross_as_16_bit_and_are_widened_on_the_host(wslib, gpu_ctx, oracle):
    """The wire format (ws_last_wire_format): 16-bit integers for every search whose kernels write the map themselves,
    into CV_64F and CV_32F buffers, pageable and pinned, plain and in bands, all views; float32 where other kernels
    read the map back (smoothFactor, varBlock) or its values are no integers (sub-pixel)."""
    import torch
    left, right, _ = make_pair(300, 140, MAXD, seed=340)
    left[60, 100] = 0
    right[70, 90] = 0
    for view, fn in ((wslib.VIEW_LEFT, oracle.block_left), (wslib.VIEW_RIGHT, oracle.block_right)):
        p = wslib.make_params(view, BS, 0, MAXD)
        want = fn(left, right, BS, 0, MAXD)
        for dtype in (np.float64, np.float32):
            out = np.full((140, 300), 123.0, dtype=dtype)
            assert host_call(wslib, gpu_ctx, p, left, right, out) == (OURS,) * 3
            assert gpu_ctx.last_wire_format() == "int16"
            assert np.array_equal(out.astype(np.float64), want)
            pin = torch.full((140, 300), 123.0, dtype=torch.float64 if dtype == np.float64 else torch.float32).pin_memory()
            how = host_call(wslib, gpu_ctx, p, left, right, pin.numpy())
            assert how[2] == "caller-pinned" and gpu_ctx.last_wire_format() == "int16"
            assert np.array_equal(pin.numpy().astype(np.float64), want)
        # padded output rows: the widening leaves the padding alone
        out = np.full((140, 320), -5.0)
        host_call(wslib, gpu_ctx, p, left, right, out, out_stride=320)
        assert np.array_equal(out[:, :300], want) and (out[:, 300:] == -5.0).all()
    pl = wslib.make_params(wslib.VIEW_LINEAR, 1, 0, MAXD)
    out = np.empty((140, 300))
    host_call(wslib, gpu_ctx, pl, left, right, out)
    assert gpu_ctx.last_wire_format() == "int16" and np.array_equal(out, oracle.linear(left, right, search_range=200))
    # float32 on the wire: smoothFactor (another kernel reads the map back), sub-pixel values
    ps = wslib.make_params(wslib.VIEW_RIGHT, BS, 0, MAXD, 0.9)
    out = np.empty((140, 300))
    host_call(wslib, gpu_ctx, ps, left, right, out)
    assert gpu_ctx.last_wire_format() == "float32" and np.array_equal(out, oracle.block_right(left, right, BS, 0, MAXD, smooth=0.9))
    pq = wslib.make_params(wslib.VIEW_LEFT, BS, 0, MAXD, 1.0, "ssd", subpixel=True)
    out = np.empty((140, 300))
    host_call(wslib, gpu_ctx, pq, left, right, out)
    assert gpu_ctx.last_wire_format() == "float32"
    assert np.abs(out - oracle.block_left(left, right, BS, 0, MAXD, subpixel=True)).max() <= 1e-4
    assert np.array_equal(out, oracle.block_left(left, right, BS, 0, MAXD, subpixel="float32"))
    # in bands (a megapixel and more): band by band through the stage, widened while the next band is searched
    big_l, big_r, _ = make_pair(1100, 1000, 32, seed=341)
    pb = wslib.make_params(wslib.VIEW_LEFT, BS, 0, 32)
    with wslib.WindowSearch(0) as ctx:
        ctx.set_host_bands(4)
        banded = np.empty((1000, 1100))
        host_call(wslib, ctx, pb, big_l, big_r, banded)
        assert ctx.last_wire_format() == "int16"
        ctx.set_host_bands(0)
        plain = np.empty((1000, 1100), dtype=np.float32)
        host_call(wslib, ctx, pb, big_l, big_r, plain)
        assert np.array_equal(banded, plain.astype(np.float64))
        rows = (500, 540)
        assert np.array_equal(plain[rows[0]:rows[1]].astype(np.float64), oracle.block_left(big_l, big_r, BS, 0, 32, rows=rows, threads=8)[rows[0]:rows[1]])


def test_values_at_the_edge_of_16_bits(wslib, gpu_ctx, oracle):
    """Stored values reach +-(width - 1) through the no-candidate fallbacks (BlockSearch.cpp:82: x, :174: -x).  A
    32767-pixel-wide image still crosses as int16 (|value| <= 32766), a wider one as float32; both maps are exact."""
    rng = np.random.default_rng(77)
    for w, wire in ((32767, "int16"), (32770, "float32")):
        left = rng.integers(1, 255, size=(8, w, 3), dtype=np.uint8)
        right = rng.integers(1, 255, size=(8, w, 3), dtype=np.uint8)
        # right view, minDisparity so large that no candidate exists: every pixel stores -x
        p = wslib.make_params(wslib.VIEW_RIGHT, 3, w + 5, w + 9)
        out = np.empty((8, w))
        host_call(wslib, gpu_ctx, p, left, right, out)
        assert gpu_ctx.last_wire_format() == wire
        assert np.array_equal(out, oracle.block_right(left, right, 3, w + 5, w + 9))
        assert out.min() == -(w - 1)
        # left view: column x = half stores half, wide disparity range
        p = wslib.make_params(wslib.VIEW_LEFT, 3, 0, 40)
        out32 = np.empty((8, w), dtype=np.float32)
        host_call(wslib, gpu_ctx, p, left, right, out32)
        assert gpu_ctx.last_wire_format() == wire
        assert np.array_equal(out32.astype(np.float64), oracle.block_left(left, right, 3, 0, 40))
    # a disparity range beyond 16 bits changes nothing: a stored value is a column difference, below the image width
    left, right, _ = make_pair(300, 40, MAXD, seed=342)
    p = wslib.make_params(wslib.VIEW_LEFT, BS, 0, 40000)
    out = np.empty((40, 300))
    host_call(wslib, gpu_ctx, p, left, right, out)
    assert gpu_ctx.last_wire_format() == "int16" and np.array_equal(out, oracle.block_left(left, right, BS, 0, 40000))
