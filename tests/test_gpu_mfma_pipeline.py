"""The pipelined steady step of the matrix-core SSD kernel (csrc/ws_march_mfma.h) where a reordered step can go wrong:
operand reads issued at the top of the step, bias quads read a tile ahead, the entering MFMAs of every tile ahead of
the leaving ones, the half merge on v_permlane32_swap.

Every case runs in a fresh child process with WS_MARCH_MFMA=1 (read once per process: the kernel is then taken below
the size rule), asserts through ws.plan and last_launch that the matrix kernel ran, and compares the whole map with
oracle.fast_left, np.array_equal:

  * tile activity boundaries.  With d_lo = 1, tile t of a column has a candidate iff D >= 32 (8 - t) - 30.  D = 97 / 98:
    the 5-tile waves have no active tile / one; D = 225 / 226: they skip one tile (the simple loop) / run the branch-free
    pipelined march; D = 33 / 34; D = 256.  All on a shape with strips of at least 2 WH = 14 rows, found by scanning
    ws.plan in the child, so that the steady phase runs for many steps;
  * strip lengths 1, 2, 3, 4 and 8, and a shape whose last strip is shorter than the others: the hand-over from phase 1
    to 2 to 3;
  * ties of every kind the merge decides: rows that repeat with a period of 4 columns and differ from row to row, every
    pixel value >= 1 (the black-pixel rule stays out), right image = left image.  Every d = 0 (mod 4) costs exactly 0, so
    equal keys meet between the registers of a tile, between the two lane halves (m and m + 4), between the tiles of a
    wave and between the two waves of a column.  Period 32: ties between tiles only;
  * a last tile with exactly 1 interior column on the tie pair (waves without columns of their own beside live ones).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, WH = 7, 7
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


def plan(maxd, shape):
    p = ws.plan(params(maxd), shape, shape)
    assert p["kernel_kind"] == 1 and p["tile_cols"] == 128 and p["threads"] == 512 and p["lds_bytes"] == 134368, p
    return p


def rows_of(p):
    return p["interior_y1"] - p["interior_y0"]


def last_strip(p):
    return rows_of(p) - (p["strips"] - 1) * p["strip_rows"]


def last_tile_cols(p):
    return (p["interior_x1"] - p["interior_x0"]) - (p["tiles"] - 1) * p["tile_cols"]


def scan_height(w, maxd, ok):
    for h in range(7, 1400):
        p = plan(maxd, (h, w, 3))
        if ok(p):
            return h, p
    raise AssertionError("no height suits %%s at width %%d" %% (case, w))


def tie_pair(w, h, period, seed):
    # rows that repeat with `period` columns and differ from row to row; no black pixel; right = left
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(1, 256, size=(h, period, 3), dtype=np.uint8)
    left = np.ascontiguousarray(np.tile(base, (1, (w + period - 1) // period, 1))[:, :w])
    assert all((left[y] != left[y + 1]).any() for y in range(h - 1))
    return left, left.copy()


kind, maxd = case["kind"], case.get("maxd", 256)
if kind == "range":
    # strips of at least 2 WH rows: the steady phase runs for at least 10 steps of every strip but the last
    w = 420
    h, p = scan_height(w, maxd, lambda p: p["strip_rows"] >= 14 and p["strips"] >= 2)
    left, right, _ = make_pair(w, h, maxd, 500 + maxd)
elif kind == "strips":
    w = 300
    h, p = scan_height(w, maxd, lambda p: p["strip_rows"] == case["rows"] and rows_of(p) >= case["rows"] and p["strips"] >= 2)
    left, right, _ = make_pair(w, h, maxd, 600 + case["rows"])
elif kind == "short_last_strip":
    w = 420
    h, p = scan_height(w, maxd, lambda p: p["strip_rows"] == 8 and 0 < last_strip(p) < 8 and p["strips"] >= 2)
    left, right, _ = make_pair(w, h, maxd, 77)
elif kind == "ties":
    w = case["width"]
    h, p = scan_height(w, maxd, lambda p: p["strip_rows"] >= 8 and p["strips"] >= 2)
    if "last_tile" in case:
        assert p["tiles"] >= 2 and last_tile_cols(p) == case["last_tile"], p
    left, right = tie_pair(w, h, case["period"], 900 + case["period"])
else:
    raise AssertionError(kind)

with ws.WindowSearch(0) as ctx:
    got = ctx.search(params(maxd), left, right)
    name = ctx.last_launch()["kernel"]
assert name == MFMA, name
np.savez(out_path, left=left, right=right, got=got, maxd=maxd, kernel=name, plan=json.dumps(p))
"""

CASES = (
    [("range_D%d" % d, {"kind": "range", "maxd": d}) for d in (33, 34, 97, 98, 225, 226, 256)]
    + [("strip_rows_%d" % r, {"kind": "strips", "rows": r}) for r in (1, 2, 3, 4, 8)]
    + [("short_last_strip", {"kind": "short_last_strip"}),
       ("ties_period_4", {"kind": "ties", "period": 4, "width": 420}),
       ("ties_period_32", {"kind": "ties", "period": 32, "width": 420}),
       # 391 = 2 * 3 (the border) + 3 * 128 + 1
       ("ties_last_tile_1_column", {"kind": "ties", "period": 4, "width": 391, "last_tile": 1})]
)


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_pipelined_step(case, oracle, tmp_path):
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, WS_MARCH_MFMA="1")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, json.dumps(case), path], check=True, env=env, timeout=300)
    z = np.load(path)
    assert str(z["kernel"]) == MFMA
    left, right, got, maxd = z["left"], z["right"], z["got"], int(z["maxd"])
    plan = json.loads(str(z["plan"]))
    assert plan["kernel_kind"] == 1, plan
    kind = case["kind"]
    if kind == "range":
        assert plan["strip_rows"] >= 2 * WH, plan
    elif kind == "strips":
        assert plan["strip_rows"] == case["rows"], plan
    elif kind == "short_last_strip":
        rows = plan["interior_y1"] - plan["interior_y0"]
        assert 0 < rows - (plan["strips"] - 1) * plan["strip_rows"] < plan["strip_rows"], plan
    want = oracle.fast_left(left, right, BS, 0, maxd, cost="ssd")
    if kind == "ties":
        period = case["period"]
        # the construction: every shift by a multiple of the period maps the left image onto the right one
        w = left.shape[1]
        assert left.min() >= 1
        for k in range(1, maxd // period + 1):
            assert np.array_equal(left[:, period * k:], right[:, :w - period * k]), k
        # ... and the reference's map is not constant over the interior: the largest valid d grows with x at the left edge
        inner = want[plan["interior_y0"]:plan["interior_y1"], plan["interior_x0"]:plan["interior_x1"]]
        assert len(np.unique(inner)) > 1, np.unique(inner)
        if "last_tile" in case:
            assert (plan["interior_x1"] - plan["interior_x0"]) - (plan["tiles"] - 1) * 128 == 1, plan
    assert got.shape == want.shape, plan
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (case, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], plan))
