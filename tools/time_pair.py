"""Pair-call timing (profiles/pair/): at config 2 (1500 x 1000, left base, 7 x 7 SAD, D = 256, 8 paths, P1 200, P2 800,
max_diff 1) the checked pair of maps by the route of a tree without the pair call -- ws_search_sgm_device for the left
view, again for the right view, then ws_lr_check_device -- next to ws_search_pair_device with the check, and the
sgm == NULL pair call next to ws_search_lr_device.  Device times are hipEvent pairs (ws_timer_*) around `--reps` calls on
the context stream after a warm-up call of the same shape.

  python tools/time_pair.py --measure pair                one process: this tree's figures, one JSON line
  python tools/time_pair.py --measure baseline --tree T   one process: the two-search route of the tree at T
  python tools/time_pair.py --baseline-tree T --rounds 3 --out profiles/pair
      alternates fresh child processes (baseline of T, this tree, `--rounds` times), takes the median of each figure over
      the rounds and writes time_pair.json.
The winner kernels themselves (ws_pair_wta_kernel here, ws_sgm_wta_kernel in both) are read from a kernel trace, run
separately: rocprofv3 --kernel-trace --stats -- python tools/time_pair.py --measure pair --reps 2."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BS, MAXD = 1500, 1000, 7, 256
SGM_SAD = (8, 200, 800)   # paths, P1, P2 (tools/time_sgm.py's config 2)
MAX_DIFF = 1.0


def device_ms(ctx, fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def measure(what, tree, reps):
    sys.path.insert(0, tree)
    import torch
    import stereo_reconstruction_amd as ws
    from stereo_reconstruction_amd.synthetic import make_pair
    ctx = ws.WindowSearch(0)
    left, right, _ = make_pair(W, H, MAXD, 2)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    raw_l, raw_r, out_l, out_r = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(4))
    pl = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, "sad")
    pr = ws.make_params(ws.VIEW_RIGHT, BS, 0, MAXD, 1.0, "sad")

    def two_searches():
        ctx.search_sgm_device(pl, tl, tr, raw_l, *SGM_SAD)
        ctx.search_sgm_device(pr, tl, tr, raw_r, *SGM_SAD)
        ctx.lr_check_device(raw_l, raw_r, out_l, out_r, MAX_DIFF)

    rows = {}
    rows["sgm_left_ms"] = device_ms(ctx, lambda: ctx.search_sgm_device(pl, tl, tr, raw_l, *SGM_SAD), reps)
    rows["sgm_right_ms"] = device_ms(ctx, lambda: ctx.search_sgm_device(pr, tl, tr, raw_r, *SGM_SAD), reps)
    rows["two_sgm_and_check_ms"] = device_ms(ctx, two_searches, reps)
    rows["two_sgm_failed"] = list(ctx.last_lr_counts())
    rows["search_lr_ms"] = device_ms(ctx, lambda: ctx.search_lr_device(pl, tl, tr, out_l, out_r, MAX_DIFF), 4 * reps)
    if what == "pair":
        rows["pair_sgm_check_ms"] = device_ms(ctx, lambda: ctx.search_pair_device(pl, tl, tr, out_l, out_r, SGM_SAD, None, MAX_DIFF), reps)
        rows["pair_sgm_failed"] = list(ctx.last_lr_counts())
        rows["pair_sgm_raw_ms"] = device_ms(ctx, lambda: ctx.search_pair_device(pl, tl, tr, out_l, out_r, SGM_SAD), reps)
        rows["pair_sgm_ratio_check_ms"] = device_ms(ctx, lambda: ctx.search_pair_device(pl, tl, tr, out_l, out_r, SGM_SAD, 15, MAX_DIFF), reps)
        rows["pair_block_check_ms"] = device_ms(ctx, lambda: ctx.search_pair_device(pl, tl, tr, out_l, out_r, None, None, MAX_DIFF), reps)
        rows["pair_sgm_check_right_base_ms"] = device_ms(ctx, lambda: ctx.search_pair_device(pr, tl, tr, out_l, out_r, SGM_SAD, None, MAX_DIFF), reps)
    torch.cuda.synchronize()
    print("TIME_PAIR " + json.dumps(rows), flush=True)


def child(what, tree, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", what, "--tree", tree, "--reps", str(reps)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if done.returncode != 0:
        raise RuntimeError("%s exited with %d:\n%s" % (" ".join(cmd), done.returncode, done.stderr[-2000:]))
    line = [x for x in done.stdout.splitlines() if x.startswith("TIME_PAIR ")][-1]
    return json.loads(line[len("TIME_PAIR "):])


def median_of(runs):
    keys = [k for k in runs[0] if isinstance(runs[0][k], (int, float))]
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}, \
           {k: [round(r[k], 4) for r in runs] for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=["pair", "baseline"], default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair"))
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, os.path.abspath(args.tree), args.reps)
    base, ours = [], []
    for _ in range(args.rounds):   # alternating fresh processes, one on the GPU at a time
        if args.baseline_tree:
            base.append(child("baseline", os.path.abspath(args.baseline_tree), args.reps))
        ours.append(child("pair", ROOT, args.reps))
    om, oall = median_of(ours)
    bm, ball = median_of(base) if base else ({}, {})
    result = {"shape": {"w": W, "h": H, "block_size": BS, "D": MAXD, "base": "left", "cost": "sad"}, "reps": args.reps,
              "rounds": args.rounds, "max_diff": MAX_DIFF, "sgm_sad": SGM_SAD, "failed_pixels": {k: ours[-1][k] for k in ("two_sgm_failed", "pair_sgm_failed")},
              "this_tree_median_ms": om, "this_tree_rounds_ms": oall, "baseline_tree_median_ms": bm, "baseline_tree_rounds_ms": ball}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_pair.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
