"""ws_batch_search_host / BatchSearch on the device: every map bit-identical to ws_search_host of that pair on one
context, whole pairs and row bands, over one to four workers sharing device 0 (more devices when the node has them)."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from stereo_reconstruction_amd.sharding import band_items
from stereo_reconstruction_amd.synthetic import TRAINING_H, make_pair

pytestmark = pytest.mark.gpu

WORKERS = ([0], [0, 0], [0, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def trainingh_pairs():
    return tuple(make_pair(w, h, 256, 500 + k)[:2] for k, (_, w, h, _) in enumerate(TRAINING_H))


@functools.lru_cache(maxsize=64)
def pair(w, h, seed, right_width=None):
    return make_pair(w, h, 96, seed, right_width=right_width)[:2]


def one_context(ctx, plist, pairs, dtype):
    if not isinstance(plist, (list, tuple)):
        plist = [plist] * len(pairs)
    return [ctx.search(p, l, r, dtype=dtype) for p, (l, r) in zip(plist, pairs)]


_want_cache = {}


def trainingh_want(wslib, ctx, view, cost, dtype, subpixel=False):
    key = (view, cost, np.dtype(dtype).str, subpixel)
    if key not in _want_cache:
        p = wslib.make_params(view, 7, 0, 256, 1.0, cost, subpixel=subpixel)
        _want_cache[key] = one_context(ctx, p, trainingh_pairs(), dtype)
    return _want_cache[key]


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("pair %d: %d pixels differ, first at %s: %r != %r" % (k, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


@pytest.fixture(scope="module")
def batches(wslib):
    made = {tuple(w): wslib.BatchSearch(w) for w in WORKERS}
    yield made
    for b in made.values():
        b.close()
    _want_cache.clear()


@pytest.mark.parametrize("workers", WORKERS, ids=lambda w: "workers%d" % len(w))
@pytest.mark.parametrize("bands", [True, False], ids=["bands", "whole"])
def test_trainingh_left_ssd_f32(wslib, gpu_ctx, batches, workers, bands):
    """BASELINE config 4's batch: the 15 trainingH shapes, 7x7 SSD, D 256, left view, float32 maps."""
    b = batches[tuple(workers)]
    assert b.workers == workers
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 256, 1.0, "ssd")
    items, banded = b.plan(p, trainingh_pairs(), bands=bands)
    assert banded == bands
    if bands:  # the assignment bench.py's launcher makes for as many ranks
        shapes = [(w, h) for _, w, h, _ in TRAINING_H]
        bi, shards = band_items(shapes, 256, len(workers), 7)
        assert items == [bi[j] + (r,) for r in range(len(workers)) for j in shards[r]]
    got = b.search(p, trainingh_pairs(), dtype=np.float32, bands=bands)
    assert b.statuses == [0] * len(got)
    assert_same(got, trainingh_want(wslib, gpu_ctx, wslib.VIEW_LEFT, "ssd", np.float32))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_trainingh_views_costs_dtypes_banded(wslib, gpu_ctx, batches, view, cost, dtype):
    v = wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT
    p = wslib.make_params(v, 7, 0, 256, 1.0, cost)
    b = batches[(0, 0, 0, 0)]
    assert b.plan(p, trainingh_pairs())[1]
    got = b.search(p, trainingh_pairs(), dtype=dtype)
    assert_same(got, trainingh_want(wslib, gpu_ctx, v, cost, dtype))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_subpixel_banded(wslib, gpu_ctx, batches, view, dtype):
    """Sub-pixel maps cross PCIe as float32 (the other wire format); cut into bands all the same."""
    v = wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT
    p = wslib.make_params(v, 7, 0, 256, 1.0, "ssd", subpixel=True)
    b = batches[(0, 0)]
    pairs = trainingh_pairs()[:5]
    items, banded = b.plan(p, pairs, min_rows=128)
    assert banded and len(items) > len(pairs)
    got = b.search(p, pairs, dtype=dtype, min_rows=128)
    assert_same(got, trainingh_want(wslib, gpu_ctx, v, "ssd", dtype, subpixel=True)[:5])


def test_mixed_batch_goes_whole_pair(wslib, gpu_ctx, batches):
    """smoothFactor 0.9, varBlock and LinearSearch in one batch: whole pairs (LPT), each map as on one context."""
    pairs = [pair(320, 200, 1), pair(288, 240, 2), pair(256, 180, 3), pair(300, 210, 4), pair(240, 160, 5)]
    plist = [wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64, 0.9),
             wslib.make_params(wslib.VIEW_RIGHT, 9, 0, 64, 0.9),
             wslib.make_params(wslib.VIEW_RIGHT, 5, 0, 48, 1.0, var_block=True, thres=19.0),
             wslib.make_params(wslib.VIEW_LINEAR, smooth_factor=1.0, linear_range=200),
             wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64, 1.0, "sad")]
    for workers in ((0,), (0, 0, 0, 0)):
        b = batches[workers]
        items, banded = b.plan(plist, pairs)
        assert not banded and sorted(it[0] for it in items) == list(range(len(pairs)))
        for dtype in (np.float32, np.float64):
            assert_same(b.search(plist, pairs, dtype=dtype), one_context(gpu_ctx, plist, pairs, dtype))


def _seam_batch(wslib, n_workers, min_rows):
    """A seeded batch whose plan cuts a band at exactly min_rows rows from a pair's top or bottom edge."""
    rng = random.Random(77 + n_workers)
    for _ in range(4000):
        n = rng.randint(1, 4)
        shapes = [(rng.randint(64, 200), rng.randint(2 * min_rows, 5 * min_rows)) for _ in range(n)]
        p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 32)
        items, banded = wslib.batch_plan(p, [(h, w) for w, h in shapes], n_workers, min_rows=min_rows)
        assert banded
        cuts = [(j, y0) for j, y0, y1, _ in items if y0 > 0]
        if any(y == min_rows or shapes[j][1] - y == min_rows for j, y in cuts):
            return shapes, items
    raise AssertionError("no seeded batch puts a cut at min_rows from an edge")


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("n_workers", [2, 4])
def test_band_seams_at_min_rows(wslib, gpu_ctx, batches, view, n_workers):
    min_rows = 24
    shapes, items = _seam_batch(wslib, n_workers, min_rows)
    v = wslib.VIEW_LEFT if view == "left" else wslib.VIEW_RIGHT
    p = wslib.make_params(v, 7, 0, 32)
    pairs = [pair(w, h, 900 + k) for k, (w, h) in enumerate(shapes)]
    b = batches[(0,) * n_workers]
    assert b.plan(p, pairs, min_rows=min_rows) == (items, True)
    want = one_context(gpu_ctx, p, pairs, np.float64)
    got = b.search(p, pairs, dtype=np.float64, min_rows=min_rows)
    for j, y0, y1, _ in items:  # the rows on both sides of every cut, then everything
        if y0 > 0:
            assert np.array_equal(got[j][y0 - 4:y0 + 4], want[j][y0 - 4:y0 + 4]), (j, y0)
    assert_same(got, want)


def test_invalid_job_leaves_every_out_untouched(wslib, gpu_ctx, batches):
    pairs = [pair(200, 120, 11), pair(180, 100, 12), pair(160, 90, 13)]
    good = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 32)
    plist = [good, good, wslib.make_params(wslib.VIEW_LEFT, 8, 0, 32)]  # even blockSize in the left view
    outs = [np.full(l.shape[:2], -12345.0, dtype=np.float64) for l, _ in pairs]
    b = batches[(0, 0)]
    with pytest.raises(wslib.WsError) as e:
        b.search(plist, pairs, outs=outs)
    assert e.value.code == -2 and "job 2" in str(e.value)
    assert b.statuses == [wslib.JOB_NOT_RUN, wslib.JOB_NOT_RUN, -2]
    for o in outs:
        assert (o == -12345.0).all()
    # a bad output buffer is refused the same way
    outs[0] = np.full((120, 199), -1.0)
    with pytest.raises(ValueError):
        b.search(good, pairs, outs=outs)
    # and the batch still works afterwards
    assert_same(b.search(good, pairs), one_context(gpu_ctx, good, pairs, np.float32))


def test_one_batch_over_growing_sizes(wslib, gpu_ctx):
    p = wslib.make_params(wslib.VIEW_RIGHT, 9, 0, 64, 1.0, "sad")
    with wslib.BatchSearch([0, 0, 0]) as b:
        for scale, n in ((1, 2), (2, 5), (4, 7), (6, 4)):
            pairs = [pair(120 * scale + 7 * k, 80 * scale + 3 * k, 300 + 10 * scale + k) for k in range(n)]
            for bands in (True, False):
                got = b.search(p, pairs, dtype=np.float64, bands=bands, min_rows=32)
                assert_same(got, one_context(gpu_ctx, p, pairs, np.float64))


def test_every_device_of_the_node(wslib, gpu_ctx):
    """devices=None: one worker per device (one on a single-GPU box)."""
    with wslib.BatchSearch() as b:
        assert b.workers == list(range(wslib.device_count()))
        p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 256)
        got = b.search(p, trainingh_pairs()[:6])
        assert_same(got, one_context(gpu_ctx, p, trainingh_pairs()[:6], np.float32))


def test_cxx_batch_search_equals_one_context(wslib, gpu_ctx, tmp_path):
    exe = str(tmp_path / "batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "batch_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    lines = []
    pairs = trainingh_pairs()[:6]
    for k, (l, r) in enumerate(pairs):
        lp, rp, op = (str(tmp_path / ("%s%d.raw" % (s, k))) for s in "lro")
        l.tofile(lp)
        r.tofile(rp)
        lines.append("%s %s %d %d %s 7 0 256 %s" % (lp, rp, l.shape[1], l.shape[0], "left" if k % 2 else "right", op))
    for head in ("1 256 0 0 0", "0 256 0 0"):
        spec = tmp_path / "spec.txt"
        spec.write_text(head + "\n" + "\n".join(lines) + "\n")
        out = subprocess.run([exe, str(spec)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("same"), out.stdout + out.stderr
        for k, (l, r) in enumerate(pairs):
            p = wslib.make_params(wslib.VIEW_LEFT if k % 2 else wslib.VIEW_RIGHT, 7, 0, 256)
            want = gpu_ctx.search(p, l, r)
            assert np.array_equal(np.fromfile(str(tmp_path / ("o%d.raw" % k)), dtype=np.float64).reshape(want.shape), want)
