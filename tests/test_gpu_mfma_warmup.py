"""The head of a strip of the matrix-core SSD kernel (csrc/ws_march_mfma.h): the steps in front of a strip's first keys
(s = -3 .. 5: three that only copy, six that copy, stage and enter rows without keys), the first output row at s = 6,
and the rows that leave the windows from s = 7 on, whose sums of squares are read back from the operand ring where the
row's entry keeps them (dwords 2 and 3 of the upper lane's part: pad that the A side multiplies by zero).

Two rewrites of that head were built and measured in profiles/mfma_warmup and are NOT in the kernel: the copies of
strip rows 0 .. 8 in one burst behind the rings' zeroing, and on top of it rows 0 .. 6 staged back to back and rows
0 .. 5 entered without a barrier per row.  Both computed the same maps on these cases and were dropped for their speed.
The cases stay for the next change to that code; they are the smallest shapes at which such a prologue can go wrong.

Every case runs in a fresh child process with WS_MARCH_MFMA=1, asserts through ws.plan and last_launch that the matrix
kernel ran, and compares the whole map with oracle.block_left, np.array_equal.  The shapes are found by scanning ws.plan
in the child:

  * strip length: strips of 1, 2, 3, 4, 5, 9, 10 and 11 rows, nsteps = rows + 6 = 7 .. 17, at least two strips each.
    With fewer than 3 rows a strip has fewer than the nine rows its head copies; up to 4 rows the steady loop
    (s + 3 < nsteps from s = 7) has no iteration and the closing phase follows the first output row directly; 9, 10 and
    11 rows are the first strips with rows 9 and later, copied in the steady phase.  Every row that leaves a window
    here was staged in front of the first keys or in the first steps behind them.  Two of the cases have a last strip
    shorter than the others.  The width (263) leaves ONE column in the last of three tiles, so three of that tile's
    four column groups are waves without columns, which stage their blocks and enter nothing;
  * one strip of one output row: height 7;
  * a last tile of 33 columns (two live column groups beside two without columns) at 2 and 9 rows;
  * a narrow range, max_disparity = 40: no tile of the first wave of a column and three of the second's four are live,
    so both take the march that skips tiles; at 2 and 11 rows;
  * device images with row strides of 7 and 11 modulo 16 and odd base offsets: the byte phases of the head's rows move
    every step and differ between the two images;
  * ties: rows of period 32 (equal keys between tiles) at 3 rows per strip.
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
import os
import sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import stereo_reconstruction_amd as ws
from mfma_inputs import range_sweep_pair, tie_ladder

BS, MFMA = 7, "ws_march_kernel<ssd,7x7,mfma>"
case, out_path = json.loads(sys.argv[1]), sys.argv[2]
MAXD = case.get("maxd", 256)
P = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, "ssd")


def plan(h, w):
    p = ws.plan(P, (h, w, 3), (h, w, 3))
    assert p["kernel_kind"] == 1 and p["tile_cols"] == 128 and p["threads"] == 512 and p["lds_bytes"] == 134368, p
    return p


def last_strip(p):
    return (p["interior_y1"] - p["interior_y0"]) - (p["strips"] - 1) * p["strip_rows"]


w, rows = case["width"], case["strip_rows"]
for h in range(7, 1400):
    p = plan(h, w)
    if p["strip_rows"] != rows:
        continue
    if case["min_strips"] == 1:      # one strip of one output row
        ok = p["strips"] == 1
    elif case.get("short_last"):     # the last strip shorter than the others
        ok = p["strips"] >= 2 and 0 < last_strip(p) < rows
    else:
        ok = p["strips"] >= 2 and last_strip(p) == rows
    if ok:
        break
else:
    raise AssertionError("no height suits %%s" %% case)
assert h * w <= 320000, (h, w)
assert p["tiles"] == case["tiles"] and (p["interior_x1"] - p["interior_x0"]) - (p["tiles"] - 1) * 128 == case["last_tile"], p

if "period" in case:
    left, right = tie_ladder(w, h, (case["period"],), 1300 + case["period"])
    assert all((left[y] != left[y + 1]).any() for y in range(h - 1))
else:
    left, right = range_sweep_pair(w, h, seed=400 + w + rows)

with ws.WindowSearch(0) as ctx:
    if case.get("device"):
        # device images without torch (its import alone takes a fresh child seconds): the HIP runtime the library
        # loaded, three calls of it, and views that answer what search_device asks of a tensor
        import ctypes
        hip = ctypes.CDLL(None)
        if not hasattr(hip, "hipMalloc"):
            hip = ctypes.CDLL("libamdhip64.so")

        def chk(rc):
            assert rc == 0, "HIP error %%d" %% rc

        class View:
            def __init__(self, ptr, shape, stride0):
                self.ptr, self.shape, self.stride0 = ptr, shape, stride0

            def data_ptr(self):
                return self.ptr

            def stride(self, i):
                assert i == 0
                return self.stride0

        def to_device(host):
            ptr = ctypes.c_void_p()
            chk(hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(host.nbytes)))
            assert ptr.value %% 16 == 0
            chk(hip.hipMemcpy(ptr, ctypes.c_void_p(host.ctypes.data), ctypes.c_size_t(host.nbytes), 1))   # host to device
            return ptr.value

        def view(img, off, stride):
            host = np.zeros(off + stride * h + 64, dtype=np.uint8)
            np.lib.stride_tricks.as_strided(host[off:], (h, 3 * w), (stride, 1))[:] = img.reshape(h, 3 * w)
            return View(to_device(host) + off, (h, w, 3), stride)

        sl, sr = case["device"]
        assert sl %% 2 == 1 and sr %% 2 == 1 and sl != sr
        tl = view(left, 5, 3 * w + (sl - 3 * w) %% 16)
        tr = view(right, 9, 3 * w + (sr - 3 * w) %% 16)
        assert tl.stride(0) %% 16 == sl and tr.stride(0) %% 16 == sr and tl.stride(0) >= 3 * w and tr.stride(0) >= 3 * w
        got32 = np.full((h, w), -7.0, dtype=np.float32)
        out = View(to_device(got32), (h, w), w)
        ctx.search_device(P, tl, tr, out, None, check=True)
        chk(hip.hipMemcpy(ctypes.c_void_p(got32.ctypes.data), ctypes.c_void_p(out.ptr), ctypes.c_size_t(got32.nbytes), 2))  # device to host
        got = got32.astype(np.float64)
    else:
        got = ctx.search(P, left, right)
    name = ctx.last_launch()["kernel"]
assert name == MFMA, name
np.savez(out_path, left=left, right=right, got=got, kernel=name, plan=json.dumps(p))
"""

W263 = {"width": 263, "tiles": 3, "last_tile": 1, "min_strips": 2}
W167 = {"width": 167, "tiles": 2, "last_tile": 33, "min_strips": 2}
CASES = (
    [("strip_rows_%d" % r, dict(W263, strip_rows=r)) for r in (1, 2, 3, 4, 9, 11)]
    + [("strip_rows_5_short_last_strip", dict(W263, strip_rows=5, short_last=True)),
       ("strip_rows_10_short_last_strip", dict(W263, strip_rows=10, short_last=True)),
       ("one_strip_one_row", dict(W263, strip_rows=1, min_strips=1)),
       ("last_tile_33_strip_rows_2", dict(W167, strip_rows=2)),
       ("last_tile_33_strip_rows_9", dict(W167, strip_rows=9)),
       ("narrow_range_strip_rows_2", dict(W263, strip_rows=2, maxd=40)),
       ("narrow_range_strip_rows_11", dict(W263, strip_rows=11, maxd=40)),
       ("device_strides_7_11_strip_rows_9", dict(W263, strip_rows=9, device=(7, 11))),
       ("ties_period_32_strip_rows_3", dict(W263, strip_rows=3, period=32))]
)


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_warmup(case, oracle, tmp_path):
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, WS_MARCH_MFMA="1")
    subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), json.dumps(case), path], check=True, env=env, timeout=300)
    z = np.load(path)
    assert str(z["kernel"]) == MFMA
    left, right, got = z["left"], z["right"], z["got"]
    plan = json.loads(str(z["plan"]))
    maxd = case.get("maxd", 256)
    assert plan["kernel_kind"] == 1 and plan["tiles"] == case["tiles"] and plan["strip_rows"] == case["strip_rows"], plan
    rows = plan["interior_y1"] - plan["interior_y0"]
    last = rows - (plan["strips"] - 1) * plan["strip_rows"]
    if case["min_strips"] == 1:
        assert left.shape[0] == WH and plan["strips"] == 1 and rows == 1, plan
    else:
        assert plan["strips"] >= 2, plan
        assert (0 < last < plan["strip_rows"]) if case.get("short_last") else last == plan["strip_rows"], plan
    # (the exact reference on its own rows in parallel: 5 s on one core for the largest image, well under one on 16)
    want = oracle.block_left(left, right, BS, 0, maxd, cost="ssd", threads=min(16, oracle.host_threads()))
    if "period" in case:
        period, w = case["period"], left.shape[1]
        assert left.min() >= 1
        for k in range(1, min(maxd, w - 1) // period + 1):
            assert np.array_equal(left[:, period * k:], right[:, :w - period * k]), k
        inner = want[plan["interior_y0"]:plan["interior_y1"], plan["interior_x0"]:plan["interior_x1"]]
        assert len(np.unique(inner)) > 1, np.unique(inner)
    assert got.shape == want.shape, plan
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (case, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], plan))
