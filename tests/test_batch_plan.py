"""ws_batch_plan (include/ws_stereo.h, "many pairs over the devices of a node") against the Python sharding it restates:
sharding.band_items for batches that can be cut into row bands, sharding.lpt_assign for whole pairs.  Host only."""
import random

import pytest

from stereo_reconstruction_amd.sharding import band_items, lpt_assign
from stereo_reconstruction_amd.synthetic import TRAINING_H

WORLDS = (1, 2, 3, 4, 8, 16, 40)


def want_bands(shapes_wh, nd, world, bs, min_rows=256):
    items, shards = band_items(shapes_wh, nd, world, bs, min_rows)
    return [items[j] + (r,) for r in range(world) for j in shards[r]]


def want_whole(out_shapes_wh, nds, world):
    shards = lpt_assign([w * h * nd for (w, h), nd in zip(out_shapes_wh, nds)], world)
    return [(j, 0, out_shapes_wh[j][1], r) for r in range(world) for j in shards[r]]


def test_trainingh_bands_equal_band_items(wslib):
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 256)
    shapes = [(w, h) for _, w, h, _ in TRAINING_H]
    for world in WORLDS:
        items, banded = wslib.batch_plan(p, [(h, w) for w, h in shapes], world)
        assert banded
        assert items == want_bands(shapes, 256, world, 7), world
        # every map row of every pair belongs to exactly one item
        for j, (w, h) in enumerate(shapes):
            rows = sorted((y0, y1) for jj, y0, y1, _ in items if jj == j)
            assert rows[0][0] == 0 and rows[-1][1] == h
            assert all(a[1] == b[0] for a, b in zip(rows, rows[1:]))


def test_trainingh_whole_pairs_equal_lpt_assign(wslib):
    shapes = [(w, h) for _, w, h, _ in TRAINING_H]
    for view, nd in ((wslib.VIEW_LEFT, 256), (wslib.VIEW_RIGHT, 256 - 16)):
        p = wslib.make_params(view, 7, 16, 256)
        for world in WORLDS:
            items, banded = wslib.batch_plan(p, [(h, w) for w, h in shapes], world, bands=False)
            assert not banded
            assert items == want_whole(shapes, [nd] * len(shapes), world), (view, world)


@pytest.mark.parametrize("seed", range(10))
def test_random_batches_equal_band_items(wslib, seed):
    """50 seeded batches per seed (500 in all): 0-20 pairs, heights near 2 * min_rows (where cuts meet the min_rows
    rule), worlds up to well above the pair count, both views and several block sizes."""
    rng = random.Random(1000 + seed)
    for _ in range(50):
        n = rng.randint(0, 20)
        min_rows = rng.choice((1, 8, 64, 256))
        bs = rng.choice((1, 3, 5, 7, 9, 17))
        view = rng.choice((wslib.VIEW_LEFT, wslib.VIEW_RIGHT))
        maxd = rng.randint(2, 300)
        mind = rng.randint(0, maxd - 1) if view == wslib.VIEW_RIGHT else 0
        nd = maxd if view == wslib.VIEW_LEFT else maxd - mind
        world = rng.randint(1, n + 8)
        shapes = [(rng.randint(40, 1500), max(1, 2 * min_rows + rng.randint(-min_rows, min_rows) + rng.randint(-3, 3)))
                  for _ in range(n)]
        p = wslib.make_params(view, bs, mind, maxd)
        items, banded = wslib.batch_plan(p, [(h, w) for w, h in shapes], world, min_rows=min_rows)
        assert banded
        assert items == want_bands(shapes, nd, world, bs, min_rows), (seed, n, world, min_rows)
        items, banded = wslib.batch_plan(p, [(h, w) for w, h in shapes], world, bands=False, min_rows=min_rows)
        assert not banded
        assert items == want_whole(shapes, [nd] * n, world)


def test_fallback_to_whole_pairs(wslib):
    """Each of these makes the batch go whole-pair (banded == 0): LPT with cost out_w * out_h * nd."""
    shapes = [(w, h) for _, w, h, _ in TRAINING_H[:6]]
    hw = [(h, w) for w, h in shapes]
    base = lambda **k: wslib.make_params(k.pop("view", wslib.VIEW_LEFT), k.pop("bs", 7), k.pop("mind", 0),
                                         k.pop("maxd", 128), **k)
    cases = {
        "mixed block sizes": [base(bs=7)] * 5 + [base(bs=9)],
        "mixed nd": [base()] * 5 + [base(maxd=64)],
        "smoothFactor 0.9": [base()] * 5 + [base(smooth_factor=0.9)],
        "varBlock": [base(view=wslib.VIEW_RIGHT)] * 5 + [base(view=wslib.VIEW_RIGHT, var_block=True)],
        "LINEAR": [base()] * 5 + [wslib.make_params(wslib.VIEW_LINEAR, linear_range=128)],
    }
    for name, plist in cases.items():
        nds = [p.linear_range if p.view == wslib.VIEW_LINEAR else p.max_disparity - (p.min_disparity if p.view else 0)
               for p in plist]
        for world in (1, 3, 8):
            items, banded = wslib.batch_plan(plist, hw, world)
            assert not banded, name
            assert items == want_whole(shapes, nds, world), (name, world)
    # unequal image heights (right image shorter): the left view's map keeps the left image's size
    p = base()
    pairs = [((h, w), (h - 2, w)) for h, w in hw]
    items, banded = wslib.batch_plan(p, pairs, 4)
    assert not banded and items == want_whole(shapes, [128] * len(shapes), 4)
    # the right view's map is the right image's size
    p = base(view=wslib.VIEW_RIGHT, maxd=128)
    pairs = [((h, w), (h, w - 10)) for h, w in hw]
    items, banded = wslib.batch_plan(p, pairs, 3, bands=False)
    assert items == want_whole([(w - 10, h) for w, h in shapes], [128] * len(shapes), 3)


def test_empty_batch(wslib):
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64)
    assert wslib.batch_plan(p, [], 4) == ([], True)
    assert wslib.batch_plan(p, [], 4, bands=False) == ([], False)


def test_argument_errors(wslib):
    import ctypes
    lib = wslib.load_library()
    p = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64)
    shapes = [(100, 200), (120, 210)]
    for kw in ({"n_workers": 0}, {"min_rows": 0}):
        args = dict(n_workers=2, min_rows=256)
        args.update(kw)
        with pytest.raises(wslib.WsError) as e:
            wslib.batch_plan(p, shapes, args["n_workers"], min_rows=args["min_rows"])
        assert e.value.code == -1
    # the lowest-index invalid job decides, and the message names it
    bad = wslib.make_params(wslib.VIEW_LEFT, 8, 0, 64)
    bad_range = wslib.make_params(wslib.VIEW_LEFT, 99, 0, 64)
    with pytest.raises(wslib.WsError) as e:
        wslib.batch_plan([p, bad_range, bad], [(100, 200)] * 3, 2)
    assert e.value.code == -1 and "job 1" in str(e.value)
    with pytest.raises(wslib.WsError) as e:
        wslib.batch_plan([p, bad, bad_range], [(100, 200)] * 3, 2)
    assert e.value.code == -2 and "job 1" in str(e.value)
    # bands must be 0 or 1; room for the items; null outputs
    jobs = (wslib._Job * 2)()
    for k, (h, w) in enumerate(shapes):
        jobs[k].params, jobs[k].left, jobs[k].right = p, wslib._shape_image((h, w)), wslib._shape_image((h, w))
    items = (wslib._BatchItem * 4)()
    n, banded = ctypes.c_int(), ctypes.c_int()
    assert lib.ws_batch_plan(jobs, 2, 2, 2, 256, items, 4, ctypes.byref(n), ctypes.byref(banded)) == -1
    assert lib.ws_batch_plan(jobs, -1, 2, 1, 256, items, 4, ctypes.byref(n), ctypes.byref(banded)) == -1
    assert lib.ws_batch_plan(jobs, 2, 2, 1, 256, None, 4, ctypes.byref(n), ctypes.byref(banded)) == -1
    assert lib.ws_batch_plan(jobs, 2, 2, 1, 256, items, 4, None, ctypes.byref(banded)) == -1
    assert lib.ws_batch_plan(jobs, 2, 2, 1, 1, items, 1, ctypes.byref(n), ctypes.byref(banded)) == -1
    want = want_bands([(w, h) for h, w in shapes], 64, 2, 7, 1)
    assert n.value == len(want) == 3  # (the count needed is still reported: one pair is cut in two)
    assert lib.ws_batch_plan(jobs, 2, 2, 1, 1, items, 4, ctypes.byref(n), ctypes.byref(banded)) == 0
    assert banded.value == 1 and [(it.job, it.y0, it.y1, it.worker) for it in items[:n.value]] == want


def test_batch_create_names_the_worker_that_failed(wslib):
    """Device 99 exists nowhere: no device at all (WS_ERR_HIP) or out of range (WS_ERR_ARG); the message names the
    worker either way, and no batch is left behind."""
    with pytest.raises(wslib.WsError) as e:
        wslib.BatchSearch([99])
    assert e.value.code in (-1, -4) and "worker 0 (device 99)" in str(e.value)
    with pytest.raises(wslib.WsError) as e:
        wslib.BatchSearch([])
    assert e.value.code == -1
