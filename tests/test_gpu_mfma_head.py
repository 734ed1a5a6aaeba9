"""The matrix-core SSD kernel's pipelined step (csrc/ws_march_mfma.h) where a rewrite of its head, its ring cursors or
its minimum can go wrong.  Of the rewrites measured in profiles/mfma_head only the minimum of a tile as one chain of
v_min3 is in the kernel; the others (A operands made in front of the barrier of the step before, the leaving MFMAs
ahead of the entering ones, cursors that count down, the operand ring's slots handed on in pairs) computed the same
maps on these cases and were dropped for their speed.  The cases stay for the next change to that code.

Every case runs in a fresh child process with WS_MARCH_MFMA=1, asserts through ws.plan and last_launch that the matrix
kernel ran, and compares the whole map with oracle.fast_left, np.array_equal.  The shapes are found by scanning ws.plan
in the child.  tests/test_gpu_mfma_pipeline.py holds the tile activity boundaries, strips of 1, 2, 3, 4 and 8 rows and
the ties on short strips; here:

  * ring positions: strips of at least 100 rows at D = 256 on a tall image of three tiles (263 columns: the raw ring of
    11 rows and the operand ring of 9 pass through all 99 relative positions).  3 * 263 = 5 (mod 16), so the byte phases
    of the host images move every step, and the last tile has ONE interior column: three of its four column groups are
    waves without columns, which advance their cursors behind the barrier and not in mid-step;
  * the same on a last tile of 33 columns (two live column groups beside two without columns);
  * byte phases on device images: the tall shape through search_device on views with row strides of 7 and 11 modulo 16
    and odd base offsets, so that phIn, phOut, phPx and phSt all move every step and differ between the two images;
  * the first and last pipelined steps: with WH = 7 the steady phase starts at step 7 and runs while s + 3 < rows + 6,
    so strips of 4, 5 and 6 rows run it for exactly 0, 1 and 2 steps (rows 5 and 6 are new; 4 is here at this width);
  * ties under the chained minimum (and any order of the two MFMAs on an accumulator): rows of period 4 (equal keys between the registers of a tile, the lane
    halves, the tiles of a wave and the two waves of a column) and period 32 (between tiles only) on strips of at least
    100 rows of a four-tile image whose last tile has one column.
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

BS, MFMA, MAXD = 7, "ws_march_kernel<ssd,7x7,mfma>", 256
case, out_path = json.loads(sys.argv[1]), sys.argv[2]
P = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, "ssd")


def plan(h, w):
    p = ws.plan(P, (h, w, 3), (h, w, 3))
    assert p["kernel_kind"] == 1 and p["tile_cols"] == 128 and p["threads"] == 512 and p["lds_bytes"] == 134368, p
    return p


def scan(w, heights, ok):
    for h in heights:
        p = plan(h, w)
        if ok(p):
            return h, p
    raise AssertionError("no height suits %%s at width %%d" %% (case, w))


w = case["width"]
if "strip_rows" in case:   # short strips: exactly these rows, at least two strips
    h, p = scan(w, range(7, 1400), lambda p: p["strip_rows"] == case["strip_rows"] and p["strips"] >= 2
                and p["interior_y1"] - p["interior_y0"] >= 2 * case["strip_rows"])
else:                      # long strips: one round of workgroups, so about 256 / tiles strips of 100 rows
    tiles = plan(64, w)["tiles"]
    h, p = scan(w, range(max(7, 100 * (256 // tiles) - 200), 40000), lambda p: p["strip_rows"] >= 100)
    assert h * w <= 4 << 20, (h, w)
assert p["tiles"] == case["tiles"] and (p["interior_x1"] - p["interior_x0"]) - (p["tiles"] - 1) * 128 == case["last_tile"], p

if "period" in case:
    left, right = tie_ladder(w, h, (case["period"],), 1200 + case["period"])
    assert all((left[y] != left[y + 1]).any() for y in range(h - 1))
else:
    left, right = range_sweep_pair(w, h, seed=300 + w + case.get("strip_rows", 0))

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

LONG = {"width": 263, "tiles": 3, "last_tile": 1}
CASES = [
    ("ring_positions_100_rows", dict(LONG)),
    ("waves_without_columns_33", {"width": 167, "tiles": 2, "last_tile": 33}),
    ("device_strides_7_11", dict(LONG, device=(7, 11))),
    ("steady_steps_0", dict(LONG, strip_rows=4)),
    ("steady_steps_1", dict(LONG, strip_rows=5)),
    ("steady_steps_2", dict(LONG, strip_rows=6)),
    # 391 = 2 * 3 (the border) + 3 * 128 + 1
    ("ties_period_4_long_strip", {"width": 391, "tiles": 4, "last_tile": 1, "period": 4}),
    ("ties_period_32_long_strip", {"width": 391, "tiles": 4, "last_tile": 1, "period": 32}),
]


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_step_head(case, oracle, tmp_path):
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, WS_MARCH_MFMA="1")
    subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), json.dumps(case), path], check=True, env=env, timeout=300)
    z = np.load(path)
    assert str(z["kernel"]) == MFMA
    left, right, got = z["left"], z["right"], z["got"]
    plan = json.loads(str(z["plan"]))
    assert plan["kernel_kind"] == 1 and plan["tiles"] == case["tiles"], plan
    assert (3 * case["width"]) % 16 != 0
    if "strip_rows" in case:
        # the steady phase runs for strip_rows - 4 steps: nsteps = rows + WH - 1, first steady s = WH, s + 3 < nsteps
        nsteps = plan["strip_rows"] + WH - 1
        assert plan["strip_rows"] == case["strip_rows"] and max(0, nsteps - 3 - WH) == case["strip_rows"] - 4, plan
    else:
        assert plan["strip_rows"] >= 100, plan
    want = oracle.fast_left(left, right, BS, 0, 256, cost="ssd")
    if "period" in case:
        period, w = case["period"], left.shape[1]
        assert left.min() >= 1
        for k in range(1, 256 // period + 1):
            assert np.array_equal(left[:, period * k:], right[:, :w - period * k]), k
        inner = want[plan["interior_y0"]:plan["interior_y1"], plan["interior_x0"]:plan["interior_x1"]]
        assert len(np.unique(inner)) > 1, np.unique(inner)
    assert got.shape == want.shape, plan
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (case, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], plan))
