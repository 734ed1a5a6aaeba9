"""The row sums of the matrix-core SSD kernel (csrc/ws_march_mfma.h) on the device: the bias words come from per-pixel
sums and a 7-pixel box (a lane a pixel, the neighbours' by DPP, chunks of 58 target centres), the stored operands are
masked, and the window's sum of squares lives in the pad of another wave's operand entry.

The matrix kernel is forced (WS_MARCH_MFMA=1, read once per process, so the searches run in child processes: one per
environment, every case of that environment in it).  Each case asserts the kernel's name and compares the whole map
with oracle.block_left, np.array_equal.  The strip length is set with WS_MFMA_STRIP_ROWS where a group says so:

  * a disparity ladder 420 columns wide, D = 256: 414 interior columns are three tiles and 30 columns, every target
    centre of a tile row wins somewhere, so every chunk of sums and every chunk boundary decides pixels; the last tile
    has three waves without columns, which still do their share of the pass;
  * left and right at the extremes and as byte and pixel checkerboards, 300 rows planned as ONE strip: the widths of
    the packed fields and the running sums modulo 2^32;
  * strips of 1, 2, 7, 8 and 9 rows: the stored sum of squares is read before any row has left, exactly at the first
    leaving row, and one past it;
  * a right image narrower and shorter than the left, down to one column: the bound of the valid centres, ring bytes
    outside the image inside windows, poisoned centres.  The CPU reference alone shows that these inputs put fallback
    pixels and real winners next to the bound;
  * strided device images at every byte phase 0 .. 15 of the raw row's start, with a row stride that is a multiple of
    16 (the phase stays) and one that is odd (it moves every step);
  * max_disparity 40 and 98: the march that skips tiles, with a first d-wave that has no live tile;
  * a tie ladder of period 32, right = left: the bias words decide nothing but must be equal where the costs are.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 7
MFMA = "ws_march_kernel<ssd,7x7,mfma>"
W = 420
LADDER_DS = list(range(1, 257, 16)) + [256]   # (a band's winners span 128 centres: steps below 128 leave no gap)

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


def checker(h, w, per_pixel, first):
    n = np.arange(3 * w)
    if per_pixel:
        n = n // 3
    row = np.where(n %% 2 == 0, first, 255 - first).astype(np.uint8)
    return np.broadcast_to(row.reshape(1, w, 3), (h, w, 3)).copy()


def images(c):
    kind = c["kind"]
    if kind == "ladder":
        return mfma_inputs.disparity_ladder(c["w"], 9, 17, c["ds"])
    if kind == "ties":
        return mfma_inputs.tie_ladder(c["w"], 9, c["periods"], 31)
    if kind == "extreme":
        left = np.full((c["h"], c["w"], 3), c["left"], dtype=np.uint8)
        right = np.full((c["h"], c["w"], 3), c["right"], dtype=np.uint8)
        return left, right
    if kind == "checker":
        return checker(c["h"], c["w"], c["per_pixel"], c["left"]), checker(c["h"], c["w"], c["per_pixel"], c["right"])
    if kind == "narrow_right":
        left, right, _ = make_pair(c["w"], c["h"], c["maxd"], 61, right_width=c["w2"], right_height=c["h2"])
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
        if "device" in c:
            import torch

            def view(img, off, stride):
                hh, ww = img.shape[:2]
                buf = torch.zeros(off + stride * hh + 64, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() %% 16 == 0
                t = torch.as_strided(buf, (hh, ww, 3), (stride, 3, 1), off)
                t.copy_(torch.from_numpy(img))
                return buf, t

            d = c["device"]
            bl, tl = view(left, d["off_left"], 3 * left.shape[1] + d["pad_left"])
            br, tr = view(right, d["off_right"], 3 * right.shape[1] + d["pad_right"])
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

SWEEP_W, SWEEP_H = 300, 45


def _pad16(w):
    """Bytes to add to 3 w for a row stride that is a multiple of 16 (and leaves room)."""
    return (-3 * w) % 16 + 16


def _phase_cases():
    cases = []
    for k in range(16):
        # base offsets k and (5 k + 3) mod 16: each image's raw rows start at every phase; the strides keep it
        cases.append(("phase_%d_stride_0_mod_16" % k,
                      {"kind": "sweep", "w": SWEEP_W, "h": SWEEP_H, "maxd": 256,
                       "device": {"off_left": (5 * k + 3) % 16, "pad_left": _pad16(SWEEP_W), "off_right": k, "pad_right": _pad16(SWEEP_W)}}))
    for k in (0, 9):
        # odd strides: the phase moves by an odd amount every row, through all 16 within a strip
        cases.append(("phase_%d_stride_odd" % k,
                      {"kind": "sweep", "w": SWEEP_W, "h": SWEEP_H, "maxd": 256,
                       "device": {"off_left": 7, "pad_left": 11 - (3 * SWEEP_W) % 2, "off_right": k, "pad_right": 5 - (3 * SWEEP_W) % 2}}))
    return cases


STRIP_HEIGHTS = {1: 27, 2: 26, 7: 27, 8: 30, 9: 33}   # interior rows 21, 20, 21, 24, 27: whole strips

# environment -> [(name, case)]
GROUPS = {
    "strips_of_16": (
        {"WS_MFMA_STRIP_ROWS": "16"},
        [("ladder_every_centre", {"kind": "ladder", "w": W, "ds": LADDER_DS, "maxd": 256}),
         ("tie_ladder_32", {"kind": "ties", "w": W, "periods": (32,) * 5, "maxd": 256}),
         ("max_disparity_40", {"kind": "sweep", "w": W, "h": SWEEP_H, "maxd": 40}),
         ("max_disparity_98", {"kind": "sweep", "w": W, "h": SWEEP_H, "maxd": 98}),
         ("narrow_right_250", {"kind": "narrow_right", "w": W, "h": 60, "w2": 250, "h2": 45, "maxd": 98}),
         ("narrow_right_150", {"kind": "narrow_right", "w": W, "h": 60, "w2": 150, "h2": 52, "maxd": 98}),
         ("narrow_right_250_all_tiles", {"kind": "narrow_right", "w": W, "h": 60, "w2": 250, "h2": 45, "maxd": 256}),
         ("narrow_right_8", {"kind": "narrow_right", "w": W, "h": 60, "w2": 8, "h2": 45, "maxd": 256}),
         ("narrow_right_1", {"kind": "narrow_right", "w": W, "h": 60, "w2": 1, "h2": 45, "maxd": 256})]
        + _phase_cases(),
    ),
    "one_strip": (
        {"WS_MFMA_STRIP_ROWS": "100000"},
        [("target_0_left_254", {"kind": "extreme", "w": 200, "h": 306, "left": 254, "right": 0, "maxd": 256}),
         ("target_255_left_1", {"kind": "extreme", "w": 200, "h": 306, "left": 1, "right": 255, "maxd": 256}),
         ("target_0_left_0", {"kind": "extreme", "w": 200, "h": 306, "left": 0, "right": 0, "maxd": 256}),
         ("target_255_left_255", {"kind": "extreme", "w": 200, "h": 306, "left": 255, "right": 255, "maxd": 256}),
         ("byte_checkerboards", {"kind": "checker", "w": 200, "h": 306, "per_pixel": False, "left": 255, "right": 0, "maxd": 256}),
         ("byte_checkerboards_equal", {"kind": "checker", "w": 200, "h": 306, "per_pixel": False, "left": 0, "right": 0, "maxd": 256}),
         ("pixel_checkerboards", {"kind": "checker", "w": 200, "h": 306, "per_pixel": True, "left": 255, "right": 255, "maxd": 256})],
    ),
}
for _rows, _h in STRIP_HEIGHTS.items():
    GROUPS["strips_of_%d" % _rows] = ({"WS_MFMA_STRIP_ROWS": str(_rows)},
                                      [("strip_rows_%d" % _rows, {"kind": "sweep", "w": SWEEP_W, "h": _h, "maxd": 256})])

_results = {}
_wants = {}


def _run(group, tmp_path_factory):
    if group not in _results:
        env_add, cases = GROUPS[group]
        path = str(tmp_path_factory.mktemp("rowsums_" + group) / "out.npz")
        env = dict(os.environ, WS_MARCH_MFMA="1", **env_add)
        subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), json.dumps(cases), path],
                       check=True, env=env, timeout=300)
        _results[group] = np.load(path)
    return _results[group]


def _want(oracle, left, right, maxd):
    """The reference map, computed once per distinct input (the phase cases share one)."""
    key = (left.shape, right.shape, maxd, hash(left.tobytes()), hash(right.tobytes()))
    if key not in _wants:
        _wants[key] = oracle.block_left(left, right, BS, 0, maxd, cost="ssd", threads=16)
    return _wants[key]


ALL = [(g, n) for g, (_, cases) in GROUPS.items() for n, _ in cases]


@pytest.mark.parametrize("group,name", ALL, ids=[n for _, n in ALL])
def test_row_sums(group, name, oracle, tmp_path_factory):
    z = _run(group, tmp_path_factory)
    case = dict(GROUPS[group][1])[name]
    left, right, got = z[name + "/left"], z[name + "/right"], z[name + "/got"]
    meta = json.loads(str(z[name + "/meta"]))
    assert meta["kernel"] == MFMA
    plan = meta["plan"]
    y0, y1 = plan["interior_y0"], plan["interior_y1"]
    rows = y1 - y0
    if group == "one_strip":
        assert plan["strips"] == 1 and plan["strip_rows"] == rows == 300, plan
    elif group == "strips_of_16":
        assert 8 <= plan["strip_rows"] <= 16 and plan["strips"] >= 3, plan
    else:
        forced = int(GROUPS[group][0]["WS_MFMA_STRIP_ROWS"])
        assert plan["strip_rows"] == forced and plan["strips"] * forced == rows and plan["strips"] >= 3, plan
    maxd = case["maxd"]
    want = _want(oracle, left, right, maxd)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first %s (got %s, want %s); %s"
                             % (name, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], plan))
    w = left.shape[1]
    inner = want[y0:y1, mfma_inputs.HALF:w - mfma_inputs.HALF]
    x = np.arange(mfma_inputs.HALF, w - mfma_inputs.HALF)[None, :]
    if name == "ladder_every_centre":
        # on the CPU reference alone: every target centre index of a tile row, 0 .. 383 = 256 + (x - 3) % 128 - (d - 1),
        # is the winner's somewhere but 0, which belongs to d = 257
        d = inner.astype(np.int64)
        ok = (d >= 1) & (d <= maxd) & (inner == d) & (inner != x)
        centre = 256 + np.broadcast_to((x - mfma_inputs.HALF) % mfma_inputs.TILE_COLS, d.shape)[ok] - (d[ok] - 1)
        assert set(np.unique(centre)) == set(range(1, 384)), sorted(set(range(1, 384)) - set(np.unique(centre)))[:10]
        assert (w - 2 * mfma_inputs.HALF) % mfma_inputs.TILE_COLS <= 32, "the last tile has waves without columns"
    if case["kind"] == "narrow_right":
        # on the CPU reference alone: the last valid target centre is column w2 - 4; a pixel none of whose candidates
        # x - d, d = 1 .. maxd, is a valid centre gets the fallback value x
        w2 = right.shape[1]
        b_lo, b_hi = mfma_inputs.HALF, w2 - 1 - mfma_inputs.HALF
        fallback = inner == x
        has_candidate = (x - 1 >= b_lo) & (x - maxd <= b_hi) & (b_hi >= b_lo)
        assert np.array_equal(fallback.all(axis=0), ~has_candidate[0]) or w2 <= 2 * mfma_inputs.HALF
        assert fallback.any(), "fallback pixels"
        if b_hi >= b_lo:
            d = inner.astype(np.int64)
            won = ~fallback & (d >= 1) & (d <= maxd)
            at_bound = won & (x - d == b_hi)
            assert at_bound.any() and (won & (x - d == b_hi - 1)).any(), "real winners at the bound and next to it"
            assert not (won & (x - d > b_hi)).any()
            if x[0, -1] - maxd > b_hi:
                # ... and side by side: the first column without a candidate follows one whose only candidate is b_hi
                edge = b_hi + maxd
                assert at_bound[:, edge - mfma_inputs.HALF].all() and fallback[:, edge + 1 - mfma_inputs.HALF].all()
        else:
            assert fallback.all(), "no valid centre at all"
    if name in ("target_0_left_254", "target_255_left_1", "byte_checkerboards", "byte_checkerboards_equal", "pixel_checkerboards"):
        assert got[y0:y1].any(), "the map is not trivially zero"
