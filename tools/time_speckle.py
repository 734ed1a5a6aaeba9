"""Speckle filter timing (profiles/speckle/): ws_filter_speckles_device on the left map of a block search, next to that
search, at config 2 (1500 x 1000, 7 x 7 SSD, D = 256) and config 5's 3840 x 2160 (9 x 9 SSD, D = 1024); the host form
(ws_filter_speckles_host, map up and down) at both; and the Teddy-H quality figures with and without the filter.

Device times are event pairs around `--reps` calls on one stream (the search: the context's timer).  The filter works
in place, so every call first restores the searched map with a device-to-device copy; that copy is timed on its own and
subtracted.  Host times are the best of `--reps` wall-clock calls.  Run the kernel trace (rocprofv3 --kernel-trace --stats) separately.

Bytes per filter: the local kernel reads the map (4 B/px) and writes the label plane (4 B/px) and, at local roots, three
more words; the size kernel reads the labels (4 B/px); the apply kernel reads the labels and the parent and count of
each pixel's root (mostly cache hits) and stores new_val into removed pixels.  About 12 B/px of compulsory traffic plus
~16 B per local root; the rates printed are 12 B/px over the measured time (the HBM peak is 8 TB/s)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import stereo_reconstruction_amd as ws  # noqa: E402
from stereo_reconstruction_amd.synthetic import make_pair  # noqa: E402

CONFIGS = {"config2": (1500, 1000, 7, 256, 2), "config5": (3840, 2160, 9, 1024, 5)}
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


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


def teddy(ctx, max_size, max_diff):
    z = np.load(os.path.join(GOLDEN, "teddyH_pair.npz"))
    nd = int(z["ndisp"])
    p = ws.make_params(ws.VIEW_LEFT, 7, 0, nd, 1.0, "ssd")
    raw = ctx.search(p, z["left"], z["right"], np.float32)
    checked, _ = ctx.search_lr(p, z["left"], z["right"], 1.0, False, dtype=np.float32)
    print("Teddy-H (%dx%d, 7 x 7 SSD, D = %d), evaldisp bad-2.0 over the kept pixels (d != 0) of the mask:" % (
        raw.shape[1], raw.shape[0], nd))
    for label, m in (("search", raw), ("search + LR check", checked)):
        for filtered in (False, True):
            out = ctx.filter_speckles(m, 0.0, max_size, max_diff) if filtered else m
            e = ws.evaldisp(out, z["gt"], z["mask"], 2.0, float(nd))
            kept = 100.0 - e["invalid"]
            print("  %-28s kept %6.2f%%  bad-2.0 on kept %6.2f%%" % (label + (" + filter" if filtered else ""), kept,
                                                                     100.0 * e["bad"] / kept if kept else 0.0))
            if filtered:
                px, regions = ctx.last_speckle_counts()
                print("  %-28s (%d pixels in %d regions removed; max_speckle_size %d, max_diff %g)" % (
                    "", px, regions, max_size, max_diff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config2,config5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-size", type=int, default=100)
    ap.add_argument("--max-diff", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    ctx = ws.WindowSearch(0)
    ms, md = args.max_size, args.max_diff
    for name in args.configs.split(","):
        w, h, bs, maxd, seed = CONFIGS[name]
        left, right, _ = make_pair(w, h, maxd, seed)
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        searched = torch.empty((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        pl = ws.make_params(ws.VIEW_LEFT, bs, 0, maxd, 1.0, "ssd")
        t_search = device_ms(ctx, lambda: ctx.search_device(pl, tl, tr, searched), max(1, args.reps // 4))
        n = w * h
        # the maps the filter sees: the search's own (few speckles on a synthetic pair), the same with 2 % of its pixels
        # replaced by random disparities (about that many singleton speckles), one region covering the whole map that is
        # removed (every local region adds into one counter), and a one-pixel serpentine (the most tile merges)
        noisy = searched.clone()
        g = torch.Generator(device="cuda").manual_seed(seed)
        hit = torch.rand((h, w), device="cuda", generator=g) < 0.02
        noisy[hit] = torch.randint(1, maxd, (int(hit.sum()),), device="cuda", generator=g).float()
        serp = np.zeros((h, w), np.float32)
        serp[0::2] = 5
        serp[1::4, -1] = 5
        serp[3::4, 0] = 5
        maps = [("searched", searched, ms), ("searched + 2% noise", noisy, ms),
                ("one region, removed", torch.full((h, w), 3.0, device="cuda"), n),
                ("serpentine, kept", torch.from_numpy(serp).cuda(), ms)]
        print("%s %dx%d bs %d D %d: search left view %.3f ms (device)" % (name, w, h, bs, maxd, t_search))
        # a stream of our own: the copies and the filters on it, timed with its events
        s = torch.cuda.Stream()
        for label, src, max_size in maps:
            work = torch.empty_like(src)
            torch.cuda.synchronize()

            def restore():
                work.copy_(src)

            def restore_and_filter():
                work.copy_(src)
                ctx.filter_speckles_device(work, 0.0, max_size, md, stream=s.cuda_stream)

            def timed(fn, reps):
                with torch.cuda.stream(s):
                    fn()
                    s.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(reps):
                        fn()
                    e1.record(s)
                    e1.synchronize()
                return e0.elapsed_time(e1) / reps

            t_copy = timed(restore, args.reps)
            t_both = timed(restore_and_filter, args.reps)
            px, regions = ctx.last_speckle_counts()
            t_filter = t_both - t_copy
            fbytes = 12 * n
            print("  %-20s filter %.4f ms = %.1f%% of the search; %.2f TB/s of 12 B/px (copy %.4f, copy + filter %.4f ms); "
                  "%d pixels in %d regions removed (max_speckle_size %d, max_diff %g)" % (
                      label, t_filter, 100 * t_filter / t_search, fbytes / t_filter / 1e9, t_copy, t_both, px, regions,
                      max_size, md))
        host_map = searched.cpu().numpy()
        t_host = host_ms(lambda: ctx.filter_speckles(host_map, 0.0, ms, md), max(2, args.reps // 4))
        print("  host form (float32 map up, filter, down) %.2f ms" % t_host, flush=True)
    teddy(ctx, ms, md)
    ctx.close()


if __name__ == "__main__":
    main()
