"""Uniqueness-ratio timing (profiles/unique/): ws_search_unique_device at config 2 (1500 x 1000, left view, 7 x 7 SAD,
D = 256) over 8-path SGM sums and on the block route (sgm == NULL), next to ws_search_sgm_device and ws_search_device of
another tree (the parent commit) at the same shape.  Device times are hipEvent pairs (ws_timer_*) around `--reps` calls on
the context stream after a warm-up call of the same shape.

  python tools/time_unique.py --measure unique              one process: this tree's figures, one JSON line
  python tools/time_unique.py --measure baseline --tree T   one process: SGM and the block search of the tree at T
  python tools/time_unique.py --baseline-tree T --rounds 3 --out profiles/unique
      alternates fresh child processes (baseline of T, this tree, `--rounds` times), takes the median of each figure over
      the rounds and writes time_unique.json.
The winner kernels themselves (ws_unique_wta_kernel here, ws_sgm_wta_kernel in the parent) are read from a kernel trace,
run separately: rocprofv3 --kernel-trace --stats -- python tools/time_unique.py --measure unique (or baseline --tree T)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BS, MAXD = 1500, 1000, 7, 256
SGM_SAD = (8, 200, 800)   # paths, P1, P2 (tools/time_sgm.py's config 2)
RATIO = 15


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
    out = torch.empty((H, W), dtype=torch.float32, device="cuda")
    p = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, "sad")
    rows = {}
    rows["sad_search_ms"] = device_ms(ctx, lambda: ctx.search_device(p, tl, tr, out), 4 * reps)
    rows["sgm_sad_8_ms"] = device_ms(ctx, lambda: ctx.search_sgm_device(p, tl, tr, out, *SGM_SAD), reps)
    rows["sgm_sad_4_p0_ms"] = device_ms(ctx, lambda: ctx.search_sgm_device(p, tl, tr, out, 4, 0, 0), reps)
    if what == "unique":
        conf = torch.empty((H, W), dtype=torch.float32, device="cuda")
        rows["unique_sgm_8_ms"] = device_ms(ctx, lambda: ctx.search_unique_device(p, tl, tr, out, RATIO, SGM_SAD, conf), reps)
        rows["unique_sgm_8_no_conf_ms"] = device_ms(ctx, lambda: ctx.search_unique_device(p, tl, tr, out, RATIO, SGM_SAD), reps)
        rows["unique_block_ms"] = device_ms(ctx, lambda: ctx.search_unique_device(p, tl, tr, out, RATIO, None, conf), reps)
        rows["unique_block_no_conf_ms"] = device_ms(ctx, lambda: ctx.search_unique_device(p, tl, tr, out, RATIO, None), reps)
        failed, nodes = ctx.last_unique_counts()
        rows["block_failed_share"] = failed / max(1, nodes)
    torch.cuda.synchronize()
    print("TIME_UNIQUE " + json.dumps(rows), flush=True)


def child(what, tree, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", what, "--tree", tree, "--reps", str(reps)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if done.returncode != 0:
        raise RuntimeError("%s exited with %d:\n%s" % (" ".join(cmd), done.returncode, done.stderr[-2000:]))
    line = [x for x in done.stdout.splitlines() if x.startswith("TIME_UNIQUE ")][-1]
    return json.loads(line[len("TIME_UNIQUE "):])


def median_of(runs):
    keys = [k for k in runs[0] if isinstance(runs[0][k], (int, float))]
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}, \
           {k: [round(r[k], 4) for r in runs] for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=["unique", "baseline"], default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unique"))
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, os.path.abspath(args.tree), args.reps)
    base, ours = [], []
    for _ in range(args.rounds):   # alternating fresh processes, one on the GPU at a time
        if args.baseline_tree:
            base.append(child("baseline", os.path.abspath(args.baseline_tree), args.reps))
        ours.append(child("unique", ROOT, args.reps))
    om, oall = median_of(ours)
    bm, ball = median_of(base) if base else ({}, {})
    result = {"shape": {"w": W, "h": H, "block_size": BS, "D": MAXD, "view": "left", "cost": "sad"}, "reps": args.reps,
              "rounds": args.rounds, "ratio": RATIO, "sgm_sad": SGM_SAD, "this_tree_median_ms": om, "this_tree_rounds_ms": oall,
              "baseline_tree_median_ms": bm, "baseline_tree_rounds_ms": ball}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_unique.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
