"""The step skeleton of the matrix-core SSD kernel (csrc/ws_march_mfma.h) where it can go wrong: raw rows centred by
their consumers, the operand pass that also forms the bias values, the roles dealt to the waves by tile share, ring
cursors advanced with a wrap, reads issued ahead of their waits, copies that may span a barrier.

Every case runs in a fresh child process with WS_MARCH_MFMA=1 (read once per process: the kernel is then taken below
the size rule), asserts that the matrix kernel ran, and compares the whole map with oracle.fast_left, np.array_equal:

  * short strips: heights, found by scanning ws.plan in the child, that give strips of 1, 2, 3 and 4 rows -- the
    look-ahead guards of a strip's end meet its first steps;
  * a last tile with exactly 1 interior column; last tiles that end 1 column past a multiple of 32 (waves without
    columns of their own beside live ones: they still prepare operand blocks);
  * a right image whose row stride is odd and whose width leaves one tile 1017 bytes of a target row, so that the
    number of 64-lane copy instructions per row (raw_dma's arithmetic, restated below) is 1 on some rows of a strip and
    2 on others, and 0 for the tile whose target columns lie wholly outside the right image;
  * max_disparity 33 and 256 on a short-strip shape;
  * black pixels on both sides, and an all-black left row inside a 1-row strip (the black-pixel test reads raw bytes;
    the wave that writes the row out is the second of a column's two).
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

_CHILD = r"""
import json
import sys
sys.path.insert(0, %r)
import numpy as np
import stereo_reconstruction_amd as ws
from stereo_reconstruction_amd.synthetic import make_pair

BS, MFMA = 7, "ws_march_kernel<ssd,7x7,mfma>"
case, out_path = json.loads(sys.argv[1]), sys.argv[2]


def params(maxd):
    return ws.make_params(ws.VIEW_LEFT, BS, 0, maxd, 1.0, "ssd")


def plan(maxd, lshape, rshape=None):
    p = ws.plan(params(maxd), lshape, rshape or lshape)
    assert p["kernel_kind"] == 1 and p["tile_cols"] == 128 and p["threads"] == 512, p
    return p


def last_tile_cols(p):
    return (p["interior_x1"] - p["interior_x0"]) - (p["tiles"] - 1) * p["tile_cols"]


def scan_height(w, maxd, strip_rows):
    for h in range(7, 600):
        p = plan(maxd, (h, w, 3))
        if p["strip_rows"] == strip_rows and p["interior_y1"] - p["interior_y0"] >= strip_rows:
            return h, p
    raise AssertionError("no height gives strips of %%d rows at width %%d" %% (strip_rows, w))


def copy_trips(addr, nbytes):
    # raw_dma (csrc/ws_march_kernel.h): the 16-byte blocks that hold a byte of the row, 64 per instruction
    if nbytes == 0:
        return 0
    blocks = ((addr & 15) + nbytes + 15) >> 4
    return (blocks + 63) >> 6


meta = {}
device = None
kind = case["kind"]
if kind == "short_strips":
    maxd, w = case["maxd"], 300
    h, p = scan_height(w, maxd, case["rows"])
    left, right, _ = make_pair(w, h, maxd, 100 + 10 * case["rows"] + maxd %% 7)
    meta["plan"] = p
elif kind == "last_tile":
    maxd, h = 256, 19
    want = case["cols"]
    for w in range(200, 600):
        p = plan(maxd, (h, w, 3))
        if p["tiles"] >= 2 and last_tile_cols(p) == want:
            break
    else:
        raise AssertionError("no width gives a last tile of %%d columns" %% want)
    left, right, _ = make_pair(w, h, maxd, 300 + want)
    meta["plan"] = p
elif kind == "copy_count":
    # left view: target centre of candidate (x, d) is column x - d of the right image, d from 0 on, window origin -3;
    # raw index 0 of a tile's target row is column tile_x0 - 256 - 3 (ws_march_mfma.h: vb0, n_b = 396 pixels per row)
    maxd, w = 256, 660
    for h in range(60, 800, 4):               # strips long enough for the steady phase, where a copy spans a barrier
        p0 = plan(maxd, (h, w, 3))
        if p0["strip_rows"] >= 8:
            break
    else:
        raise AssertionError("no height gives strips of 8 rows at width %%d" %% w)
    x0 = p0["interior_x0"]
    w2 = (x0 + 2 * 128 - 256 - 3) + 339      # tile 2 then sees 339 pixels = 1017 bytes of a right row
    h2 = h
    p = plan(maxd, (h, w, 3), (h2, w2, 3))
    assert p["interior_x0"] == x0 and p["tiles"] == 6, p
    stride2, off2 = 3 * w2 + 2, 5            # an odd row stride: the phase of a row's first byte walks through 0 .. 15
    assert stride2 %% 2 == 1
    left, right, _ = make_pair(w, h, maxd, 41, right_width=w2, right_height=h2)
    device = {"left": (0, 3 * w + 16), "right": (off2, stride2)}
    meta["plan"] = p
    meta["w2"] = w2
elif kind == "black":
    maxd, w = 256, 300
    h, p = scan_height(w, maxd, 1)
    left, right, _ = make_pair(w, h, maxd, 77)
    y = p["interior_y0"] + (p["interior_y1"] - p["interior_y0"]) // 2
    left[y] = 0                               # an all-black left row: the whole output row of a 1-row strip
    left[p["interior_y0"], 40:90] = 0
    left[:, 200:203] = 0
    right[y - 1, 100:180] = 0
    right[:, 30:33] = 0
    meta["plan"] = p
    meta["black_row"] = int(y)
else:
    raise AssertionError(kind)

with ws.WindowSearch(0) as ctx:
    if device is None:
        got = ctx.search(params(maxd), left, right)
    else:
        import torch

        def view(img, off, stride):
            hh, ww = img.shape[:2]
            buf = torch.zeros(off + stride * hh + 64, dtype=torch.uint8, device="cuda")
            t = torch.as_strided(buf, (hh, ww, 3), (stride, 3, 1), off)
            t.copy_(torch.from_numpy(img))
            return buf, t

        bl, tl = view(left, *device["left"])
        br, tr = view(right, *device["right"])
        if kind == "copy_count":
            # the property this input is chosen for, from raw_dma's own arithmetic on the addresses the kernel will see
            p = meta["plan"]
            w2, stride2 = meta["w2"], tr.stride(0)
            per_tile = []
            for ti in range(p["tiles"]):
                c0 = p["interior_x0"] + 128 * ti - 256 - 3
                v_lo, v_hi = max(0, -c0), max(max(0, -c0), min(396, w2 - c0))
                nbytes = 3 * (v_hi - v_lo)
                strips = []
                for si in range(p["strips"]):
                    ys = p["interior_y0"] + si * p["strip_rows"]
                    ye = min(ys + p["strip_rows"], p["interior_y1"])
                    rows = range(ys - 3, ye + 3)      # the window rows the strip copies
                    strips.append(sorted({copy_trips(tr.data_ptr() + r * stride2 + 3 * (c0 + v_lo), nbytes) for r in rows}))
                per_tile.append((nbytes, strips))
            meta["copy_trips"] = per_tile
            assert 1010 <= per_tile[2][0] <= 1023, per_tile
            assert any(s == [1, 2] for s in per_tile[2][1]), per_tile          # 1 and 2 instructions within one strip
            assert per_tile[-1][0] == 0 and all(s == [0] for s in per_tile[-1][1]), per_tile   # wholly outside: none
        out = torch.full((left.shape[0], left.shape[1]), -7.0, dtype=torch.float32, device="cuda")
        ctx.search_device(params(maxd), tl, tr, out, None)
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
    name = ctx.last_launch()["kernel"]
assert name == MFMA, name
np.savez(out_path, left=left, right=right, got=got, maxd=maxd, kernel=name, meta=json.dumps(meta))
"""

CASES = (
    [("strip_rows_%d" % r, {"kind": "short_strips", "rows": r, "maxd": 256}) for r in (1, 2, 3, 4)]
    + [("last_tile_1_column", {"kind": "last_tile", "cols": 1}),
       ("last_tile_33_columns", {"kind": "last_tile", "cols": 33}),
       ("last_tile_97_columns", {"kind": "last_tile", "cols": 97}),
       ("copy_count_varies", {"kind": "copy_count"}),
       # the D range on a short-strip shape: max_disparity 256 is strip_rows_2 above, 33 here
       ("maxd_33_strip_rows_2", {"kind": "short_strips", "rows": 2, "maxd": 33}),
       ("black_pixels", {"kind": "black"})]
)


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_step_skeleton(case, oracle, tmp_path):
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, WS_MARCH_MFMA="1")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, json.dumps(case), path], check=True, env=env, timeout=300)
    z = np.load(path)
    assert str(z["kernel"]) == MFMA
    left, right, got, maxd = z["left"], z["right"], z["got"], int(z["maxd"])
    meta = json.loads(str(z["meta"]))
    if case["kind"] == "short_strips":
        assert meta["plan"]["strip_rows"] == case["rows"], meta
    want = oracle.fast_left(left, right, BS, 0, maxd, cost="ssd")
    assert got.shape == want.shape, meta
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (case, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], meta))
    if case["kind"] == "black":
        assert not got[meta["black_row"]].any(), "an all-black left row gives an all-zero output row"
