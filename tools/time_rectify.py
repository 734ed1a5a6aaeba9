"""Developer tool: time the rectification path on one MI355X.

  * ws_rectify_device on 1500 x 1000 and 3840 x 2160 CV_8UC3 images under a rectifying homography: device time per
    launch from a HIP event pair around `reps` back-to-back launches on the context stream (best of 5 windows, after
    warm-up), against the byte floor (bytes read + written at 6.0 TB/s);
  * ws_search_unrectified_host against ws_search_host on the same rectified sizes at config 2 (7 x 7 SSD, D = 256,
    left view): host wall time of the synchronous calls (median of `calls`, after warm-up).  The difference is what
    the unrectified call adds: two rectify kernels, the nearest warp back, and the larger uploads / download.

usage: time_rectify.py [reps] [calls]   (prints one line per measurement and a JSON line with every number)
       time_rectify.py launch [n]       (only n launches of the 4K warp, no timing: the program for a counter run,
                                         rocprofv3 --pmc <counters> -- python tools/time_rectify.py launch 20)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import rectify_ref as rr
import stereo_reconstruction_amd as ws
from stereo_reconstruction_amd.synthetic import make_pair

HBM_BYTES_PER_S = 6.0e12


def rectify_ms(ctx, w, h, reps):
    img = np.random.default_rng(w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    H = rr.rectifying_homography(w, h, 0.9, 0.006, (1.5e-6, -1e-6), 1.0, (3.5, -2.25))
    rh, rw = ws.rectified_size(H, (h, w))
    src = torch.from_numpy(img).cuda()
    dst = torch.empty((rh, rw, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the context's stream is not ordered against torch's: the upload is through first)
    for _ in range(5):
        ctx.rectify_device(src, H, dst)
    ctx.device_status()
    best = 1e9
    for _ in range(5):
        ctx.timer_begin()
        for _ in range(reps):
            ctx.rectify_device(src, H, dst)
        best = min(best, ctx.timer_end() / reps)
    nbytes = 3 * (w * h + rw * rh)
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    return {"src": [w, h], "dst": [rw, rh], "ms": best, "bytes": nbytes, "floor_ms": floor_ms,
            "x_floor": best / floor_ms, "GBps": nbytes / best / 1e6}


def host_call_ms(fn, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def launch_only(n):
    h, w = 2160, 3840
    img = np.random.default_rng(w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    H = rr.rectifying_homography(w, h, 0.9, 0.006, (1.5e-6, -1e-6), 1.0, (3.5, -2.25))
    rh, rw = ws.rectified_size(H, (h, w))
    with ws.WindowSearch(0) as ctx:
        src = torch.from_numpy(img).cuda()
        dst = torch.empty((rh, rw, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(n):
            ctx.rectify_device(src, H, dst)
        ctx.device_status()
    print("%d launches of ws_rectify_kernel %dx%d -> %dx%d" % (n, w, h, rw, rh))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "launch":
        launch_only(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "calls": calls}
    with ws.WindowSearch(0) as ctx:
        for w, h in ((1500, 1000), (3840, 2160)):
            r = rectify_ms(ctx, w, h, reps)
            res["rectify_%dx%d" % (w, h)] = r
            print("ws_rectify_device %dx%d -> %dx%d: %.4f ms  (%.0f GB/s; byte floor %.4f ms at 6 TB/s, %.2fx)" % (
                w, h, r["dst"][0], r["dst"][1], r["ms"], r["GBps"], r["floor_ms"], r["x_floor"]), flush=True)
        left, right, _ = make_pair(1500, 1000, 256, seed=2)
        H = rr.rectifying_homography(1500, 1000, 0.8, 0.004, (1.2e-5, -0.8e-5), 1.0, (4.0, -3.0))
        Hp = rr.rectifying_homography(1500, 1000, 0.6, -0.003, (0.9e-5, 0.5e-5), 0.985, (-2.0, 1.5))
        p = ws.make_params(ws.VIEW_LEFT, 7, 0, 256, 1.0, "ssd")
        _, rl, rrt = ctx.search_unrectified(p, left, right, H, Hp, rectified=True)
        out = np.empty(rl.shape[:2], dtype=np.float64)
        unrect = host_call_ms(lambda: ctx.search_unrectified(p, left, right, H, Hp), calls)
        plain = host_call_ms(lambda: ctx.search(p, rl, rrt, out=out), calls)
        res["config2_unrectified_host_ms"] = {"median": unrect[0], "min": unrect[1], "sizes": [list(left.shape[:2]), list(rl.shape[:2]), list(rrt.shape[:2])]}
        res["config2_search_host_ms"] = {"median": plain[0], "min": plain[1], "sizes": [list(rl.shape[:2]), list(rrt.shape[:2])]}
        print("config 2 ws_search_unrectified_host %dx%d (rectified %dx%d / %dx%d): median %.3f ms (min %.3f)" % (
            left.shape[1], left.shape[0], rl.shape[1], rl.shape[0], rrt.shape[1], rrt.shape[0], *unrect), flush=True)
        print("config 2 ws_search_host on the rectified pair: median %.3f ms (min %.3f); the unrectified call adds %.3f ms" % (
            *plain, unrect[0] - plain[0]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
