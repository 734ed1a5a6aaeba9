"""Semi-global matching timing (profiles/sgm/): ws_search_sgm_device next to the block search it aggregates, at config 2
(1500 x 1000, 7 x 7 SAD, D = 256, 4 and 8 paths), Teddy-H (900 x 750, 5 x 5 SAD, D = 128, 8 paths) and 3840 x 2160
(9 x 9 SAD, D = 256, 8 paths).  Device times are hipEvent pairs around `--reps` calls on the context stream.  Run the
kernel trace (rocprofv3 --kernel-trace --stats) separately.

Bytes per call (the floor of the chosen storage: C in cb bytes, S in sb bytes, N pixels, D disparities): the cost kernel
writes C once (N D cb); the first path reads C and writes S (N D (cb + sb)), every further path reads C and S and writes S
(N D (cb + 2 sb)); the winner reads S once (N D sb).  The images, the candidate plane and the map are small beside it.
Achieved rates are those bytes over the measured time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import stereo_reconstruction_amd as ws  # noqa: E402
from stereo_reconstruction_amd.synthetic import make_pair  # noqa: E402

# name: (w, h, block_size, maxD, paths list, p1, p2)
CONFIGS = {"config2": (1500, 1000, 7, 256, (4, 8), 200, 800), "teddyH": (900, 750, 5, 128, (8,), 600, 2400),
           "4k": (3840, 2160, 9, 256, (8,), 300, 1200)}


def device_ms(ctx, fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def floor_bytes(n, d, paths, cb, sb):
    return n * d * (cb + (cb + sb) + (paths - 1) * (cb + 2 * sb) + sb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config2,teddyH,4k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    ctx = ws.WindowSearch(0)
    rows = []
    for name in args.configs.split(","):
        w, h, bs, maxd, paths_list, p1, p2 = CONFIGS[name]
        if name == "teddyH":
            z = np.load(os.path.join(ROOT, "tests", "golden", "teddyH_pair.npz"))
            left, right = z["left"], z["right"]
        else:
            left, right, _ = make_pair(w, h, maxd, 2)
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        p = ws.make_params(ws.VIEW_LEFT, bs, 0, maxd, 1.0, "sad")
        t_block = device_ms(ctx, lambda: ctx.search_device(p, tl, tr, out), args.reps)
        for paths in paths_list:
            t = device_ms(ctx, lambda: ctx.search_sgm_device(p, tl, tr, out, paths, p1, p2), args.reps)
            nd = min(maxd, w - 1 - 2 * ((bs - 1) // 2))
            cmax = 3 * 255 * bs * bs
            cb = 2 if cmax <= 0xFFFF else 4
            sb = 4 if paths * (cmax + p2) <= 0xFFFFFFFF else 8
            fb = floor_bytes(w * h, nd, paths, cb, sb)
            row = {"config": name, "w": w, "h": h, "block_size": bs, "D": nd, "paths": paths, "p1": p1, "p2": p2,
                   "sgm_ms": round(t, 3), "block_search_ms": round(t_block, 3), "cost_bytes": cb, "sum_bytes": sb,
                   "floor_GB": round(fb / 1e9, 2), "achieved_TBps": round(fb / (t * 1e-3) / 1e12, 2),
                   "scratch_GB": round(ws.sgm_scratch_bytes(p, left, right, paths, p1, p2) / 1e9, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del tl, tr, out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
