"""The packed keys of the matrix-core SSD kernel (csrc/ws_march_mfma.h) on the device: two keys per v_lshl_add_u64, 3-bit
pair tags, two minimum chains per tile, offsets that keep every word non-negative.

The matrix kernel is forced (WS_MARCH_MFMA=1, read once per process, so the searches run in child processes: one per
environment, every case of that environment in it).  Each case asserts the kernel's name and compares the whole map
with oracle.block_left, np.array_equal.  At these sizes the strip model would cut every image into strips of one row,
so the strip length is set with WS_MFMA_STRIP_ROWS: up to 16 rows (a strip's head, the pipelined steady steps and its end,
three strips and more, the last one shorter) unless a case says otherwise:

  * tie ladders (tests/mfma_inputs.py) of periods 1, 2, 4, 8, 16, 32, 64, 96: periods 1 and 2 decide between the two
    words of a pair, 4 and 8 between pairs and lane halves, the rest between tiles and d-waves;
  * all-0 and all-255 target images against a left image of the other extreme, 300 rows planned as ONE strip
    (WS_MFMA_STRIP_ROWS): E(v) and the bias sums run to +-2688 per row for 306 rows, every valid candidate ties and
    everything else is poisoned.  A left image of zeros is black everywhere (the map is zeros whatever the keys do), so
    each extreme is also run with a left image one step off it (1 and 254);
  * a right image narrower than the left: the invalid-centre poison alone (max_disparity 256) and together with the
    range poison (max_disparity 40);
  * max_disparity 1, 2, 33, 34, 255, 256 on one pair in which every candidate wins somewhere;
  * a strided device image on both sides;
  * the tile-skipping march (max_disparity 40 on the tie ladder: the 5-tile waves skip tiles);
  * strips of one row (WS_MFMA_STRIP_ROWS=1): a strip's only keys are those of PHASE 1's simple tile loop.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 7
MFMA = "ws_march_kernel<ssd,7x7,mfma>"
W = 390

_CHILD = r"""
import json
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import stereo_reconstruction_amd as ws
from stereo_reconstruction_amd.synthetic import make_pair
import mfma_inputs

BS, MFMA = 7, "ws_march_kernel<ssd,7x7,mfma>"
cases, out_path = json.loads(sys.argv[1]), sys.argv[2]


def params(maxd):
    return ws.make_params(ws.VIEW_LEFT, BS, 0, maxd, 1.0, "ssd")


def images(c):
    kind = c["kind"]
    if kind == "ties":
        return mfma_inputs.tie_ladder(c["w"], 9, c["periods"], 31)
    if kind == "extreme":
        left = np.full((c["h"], c["w"], 3), c["left"], dtype=np.uint8)
        right = np.full((c["h"], c["w"], 3), c["right"], dtype=np.uint8)
        return left, right
    if kind == "narrow_right":
        left, right, _ = make_pair(c["w"], c["h"], 256, 61, right_width=c["w2"])
        return left, right
    if kind == "sweep":
        return mfma_inputs.range_sweep_pair(c["w"], c["h"])
    raise AssertionError(kind)


out = {}
with ws.WindowSearch(0) as ctx:
    for name, c in cases:
        left, right = images(c)
        maxd = c["maxd"]
        p = ws.plan(params(maxd), left.shape, right.shape)
        assert p["kernel_kind"] == 1 and p["threads"] == 512, (name, p)
        if c.get("device"):
            import torch

            def view(img, off, stride):
                hh, ww = img.shape[:2]
                buf = torch.zeros(off + stride * hh + 64, dtype=torch.uint8, device="cuda")
                t = torch.as_strided(buf, (hh, ww, 3), (stride, 3, 1), off)
                t.copy_(torch.from_numpy(img))
                return buf, t

            bl, tl = view(left, 7, 3 * left.shape[1] + 11)
            br, tr = view(right, 5, 3 * right.shape[1] + 2)
            o = torch.full((left.shape[0], left.shape[1]), -7.0, dtype=torch.float32, device="cuda")
            ctx.search_device(params(maxd), tl, tr, o, None)
            torch.cuda.synchronize()
            got = o.cpu().numpy().astype(np.float64)
        else:
            got = ctx.search(params(maxd), left, right)
        kernel = ctx.last_launch()["kernel"]
        assert kernel == MFMA, (name, kernel)
        out[name + "/left"], out[name + "/right"], out[name + "/got"] = left, right, np.asarray(got, dtype=np.float64)
        out[name + "/meta"] = json.dumps({"kernel": kernel, "plan": p})
np.savez(out_path, **out)
"""

PERIODS = (1, 2, 4, 8, 16, 32, 64, 96)

# environment -> [(name, case)]
GROUPS = {
    "strips_of_16": (
        {"WS_MFMA_STRIP_ROWS": "16"},
        [("tie_ladders", {"kind": "ties", "w": W, "periods": PERIODS, "maxd": 256}),
         ("tile_skipping_march", {"kind": "ties", "w": W, "periods": PERIODS[:6], "maxd": 40}),
         ("narrow_right_centre_poison", {"kind": "narrow_right", "w": W, "h": 40, "w2": 250, "maxd": 256}),
         ("narrow_right_both_poisons", {"kind": "narrow_right", "w": W, "h": 40, "w2": 250, "maxd": 40}),
         ("strided_device_images", {"kind": "sweep", "w": 300, "h": 45, "maxd": 256, "device": True})]
        + [("max_disparity_%d" % d, {"kind": "sweep", "w": 300, "h": 45, "maxd": d}) for d in (1, 2, 33, 34, 255, 256)],
    ),
    "one_strip": (
        {"WS_MFMA_STRIP_ROWS": "100000"},
        [("target_0_left_255", {"kind": "extreme", "w": 200, "h": 306, "left": 255, "right": 0, "maxd": 256}),
         ("target_255_left_0", {"kind": "extreme", "w": 200, "h": 306, "left": 0, "right": 255, "maxd": 256}),
         ("target_0_left_254", {"kind": "extreme", "w": 200, "h": 306, "left": 254, "right": 0, "maxd": 256}),
         ("target_255_left_1", {"kind": "extreme", "w": 200, "h": 306, "left": 1, "right": 255, "maxd": 256})],
    ),
    "one_row_strips": (
        {"WS_MFMA_STRIP_ROWS": "1"},
        [("phase_1_only", {"kind": "sweep", "w": 300, "h": 27, "maxd": 256})],
    ),
}

_results = {}


def _run(group, tmp_path_factory):
    if group not in _results:
        env_add, cases = GROUPS[group]
        path = str(tmp_path_factory.mktemp("keys64_" + group) / "out.npz")
        env = dict(os.environ, WS_MARCH_MFMA="1", **env_add)
        subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), json.dumps(cases), path],
                       check=True, env=env, timeout=300)
        _results[group] = np.load(path)
    return _results[group]


ALL = [(g, n) for g, (_, cases) in GROUPS.items() for n, _ in cases]


@pytest.mark.parametrize("group,name", ALL, ids=[n for _, n in ALL])
def test_packed_keys(group, name, oracle, tmp_path_factory):
    z = _run(group, tmp_path_factory)
    case = dict(GROUPS[group][1])[name]
    left, right, got = z[name + "/left"], z[name + "/right"], z[name + "/got"]
    meta = json.loads(str(z[name + "/meta"]))
    assert meta["kernel"] == MFMA
    plan = meta["plan"]
    rows = plan["interior_y1"] - plan["interior_y0"]
    if group == "one_strip":
        assert plan["strips"] == 1 and plan["strip_rows"] == rows == 300, plan
    if group == "strips_of_16":
        assert 8 <= plan["strip_rows"] <= 16 and plan["strips"] >= 3, plan   # (the rows are dealt evenly: 12 .. 14 here)
    if group == "one_row_strips":
        assert plan["strip_rows"] == 1 and plan["strips"] == rows, plan
    want = oracle.block_left(left, right, BS, 0, case["maxd"], cost="ssd", threads=8)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (name, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], plan))
    if name in ("target_0_left_254", "target_255_left_1", "target_0_left_255"):
        assert got[plan["interior_y0"]:plan["interior_y1"]].any(), "the map is not trivially zero"
