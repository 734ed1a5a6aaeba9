"""Left-right check timing (profiles/lr/): ws_lr_check_device without and with the fill, next to the two block searches it
checks, and ws_search_lr_host against two ws_search_host calls, at config 2 (1500 x 1000, 7 x 7 SSD, D = 256) and config 5's
3840 x 2160 (9 x 9 SSD, D = 1024).  Device times are hipEvent pairs around `--reps` calls on the context stream; host
times are the best of `--reps` wall-clock calls.  Run the kernel trace (rocprofv3 --kernel-trace --stats) separately.

Bytes per check: each map is read once (4 B/px), its partner gathered from the same row (4 B/px, mostly cache hits),
the output written (4 B/px) and, with the fill, one state byte written; the fill reads the state bytes twice and moves
20 B per failed pixel (two source reads, two writes and one read back of the pixel itself).  Achieved rates are those
bytes over the measured time, against the 8 TB/s HBM peak."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import stereo_reconstruction_amd as ws  # noqa: E402
from stereo_reconstruction_amd.synthetic import make_pair  # noqa: E402

CONFIGS = {"config2": (1500, 1000, 7, 256, 2), "config5": (3840, 2160, 9, 1024, 5)}
HBM_PEAK = 8.0e12


def device_ms(ctx, fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def host_ms(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config2,config5")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    ctx = ws.WindowSearch(0)
    for name in args.configs.split(","):
        w, h, bs, maxd, seed = CONFIGS[name]
        left, right, _ = make_pair(w, h, maxd, seed)
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        maps = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        pl = ws.make_params(ws.VIEW_LEFT, bs, 0, maxd, 1.0, "ssd")
        pr = ws.make_params(ws.VIEW_RIGHT, bs, 0, maxd, 1.0, "ssd")
        t_left = device_ms(ctx, lambda: ctx.search_device(pl, tl, tr, maps[0]), max(1, args.reps // 4))
        t_right = device_ms(ctx, lambda: ctx.search_device(pr, tl, tr, maps[1]), max(1, args.reps // 4))
        px = 2 * w * h
        t_check = device_ms(ctx, lambda: ctx.lr_check_device(maps[0], maps[1], maps[2], maps[3], 1.0, False), args.reps)
        failed = sum(ctx.last_lr_counts())
        t_fill = device_ms(ctx, lambda: ctx.lr_check_device(maps[0], maps[1], maps[2], maps[3], 1.0, True), args.reps)
        check_bytes, check_fill_bytes = px * 12, px * 13 + px * 2 + failed * 20
        print("%s %dx%d bs %d D %d: %d of %d pixels fail (max_diff 1)" % (name, w, h, bs, maxd, failed, px))
        print("  search left view %.3f ms, right view %.3f ms (device)" % (t_left, t_right))
        print("  check            %.4f ms  %.1f%% of the left search; %.2f TB/s = %.0f%% of 8 TB/s (%d B)" % (
            t_check, 100 * t_check / t_left, check_bytes / t_check / 1e9, 100 * check_bytes / (t_check * 1e-3) / HBM_PEAK, check_bytes))
        print("  check + fill     %.4f ms  %.1f%% of the left search; %.2f TB/s = %.0f%% of 8 TB/s (%d B)" % (
            t_fill, 100 * t_fill / t_left, check_fill_bytes / t_fill / 1e9, 100 * check_fill_bytes / (t_fill * 1e-3) / HBM_PEAK,
            check_fill_bytes))
        reps = max(2, args.reps // 4)
        t_two = host_ms(lambda: (ctx.search(pl, left, right, np.float64), ctx.search(pr, left, right, np.float64)), reps)
        t_lr = host_ms(lambda: ctx.search_lr(pl, left, right, 1.0, False, np.float64), reps)
        t_lr_fill = host_ms(lambda: ctx.search_lr(pl, left, right, 1.0, True, np.float64), reps)
        print("  host, float64 out: two ws_search_host %.2f ms; ws_search_lr_host %.2f ms, with fill %.2f ms" % (
            t_two, t_lr, t_lr_fill), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
