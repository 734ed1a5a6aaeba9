"""Census-cost timing (profiles/census/): the census transform per image, the census block search for both costs and
SGM over 9x7, at config 2 (1500 x 1000, 7 x 7 block, D = 256, left view), next to the SAD and SSD block search and
SGM-over-SAD of another tree (the parent commit) at the same shapes.  Device times are hipEvent pairs (ws_timer_*) around
`--reps` calls on the context stream after a warm-up call of the same shape.

  python tools/time_census.py --measure census            one process: this tree's census figures, one JSON line each
  python tools/time_census.py --measure baseline --tree T  one process: SAD / SSD / SGM-over-SAD of the tree at T
  python tools/time_census.py --baseline-tree T --rounds 3 --out profiles/census
      alternates fresh child processes (baseline of T, census of this tree, `--rounds` times), takes the median of each
      figure over the rounds and writes time_census.json (profiles/census/README.md is written from it).
Run the kernel trace (rocprofv3 --kernel-trace --stats -- python tools/time_census.py --measure census) separately."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BS, MAXD = 1500, 1000, 7, 256
SGM_CENSUS = (8, 10, 120)   # paths, P1, P2 over 9x7 descriptors
SGM_SAD = (8, 200, 800)     # ... over SAD (tools/time_sgm.py's config 2)
# from the build (hipcc -Rpass-analysis=kernel-resource-usage on csrc/ws_ct.hip): the match kernel, winner-take-all sink
MATCH_KERNEL_BUILD = {"vgprs": 254, "waves_per_simd": 2, "lds_bytes": 48896}


def device_ms(ctx, fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def measure(what, tree, reps):
    sys.path.insert(0, tree)
    import numpy as np  # noqa: F401
    import torch
    import stereo_reconstruction_amd as ws
    from stereo_reconstruction_amd.synthetic import make_pair
    ctx = ws.WindowSearch(0)
    left, right, _ = make_pair(W, H, MAXD, 2)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.empty((H, W), dtype=torch.float32, device="cuda")
    rows = {}

    def search(cost):
        p = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, cost)
        return device_ms(ctx, lambda: ctx.search_device(p, tl, tr, out), reps)

    def sgm(cost, paths, p1, p2):
        p = ws.make_params(ws.VIEW_LEFT, BS, 0, MAXD, 1.0, cost)
        return device_ms(ctx, lambda: ctx.search_sgm_device(p, tl, tr, out, paths, p1, p2), max(2, reps // 4))

    if what == "baseline":
        rows["sad_search_ms"] = search("sad")
        rows["ssd_search_ms"] = search("ssd")
        rows["sgm_sad_8_ms"] = sgm("sad", *SGM_SAD)
        rows["sgm_sad_4_p0_ms"] = sgm("sad", 4, 0, 0)
    else:
        desc = torch.empty((H, W), dtype=torch.int64, device="cuda")
        for cost in ("census5x5", "census9x7"):
            rows["transform_%s_ms" % cost] = device_ms(ctx, lambda: ctx.census_transform_device(tl, cost, desc), reps)
            rows["search_%s_ms" % cost] = search(cost)
        ctx.set_profiling(True)
        for cost in ("census5x5", "census9x7"):
            search(cost)
            rows["match_kernel_%s_ms" % cost] = ctx.last_kernel_ms()
        ctx.set_profiling(False)
        rows["launch"] = ctx.last_launch()
        rows["sgm_census9x7_8_ms"] = sgm("census9x7", *SGM_CENSUS)
        rows["sgm_census9x7_4_p0_ms"] = sgm("census9x7", 4, 0, 0)
        rows["sad_search_ms"] = search("sad")
        rows["ssd_search_ms"] = search("ssd")
    torch.cuda.synchronize()
    print("TIME_CENSUS " + json.dumps(rows), flush=True)


def child(what, tree, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", what, "--tree", tree, "--reps", str(reps)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if done.returncode != 0:
        raise RuntimeError("%s exited with %d:\n%s" % (" ".join(cmd), done.returncode, done.stderr[-2000:]))
    text = done.stdout
    line = [x for x in text.splitlines() if x.startswith("TIME_CENSUS ")][-1]
    return json.loads(line[len("TIME_CENSUS "):])


def median_of(runs):
    keys = [k for k in runs[0] if isinstance(runs[0][k], (int, float))]
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}, \
           {k: [round(r[k], 4) for r in runs] for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=["census", "baseline"], default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census"))
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, os.path.abspath(args.tree), args.reps)
    base, ours = [], []
    for _ in range(args.rounds):   # alternating fresh processes, one on the GPU at a time
        if args.baseline_tree:
            base.append(child("baseline", os.path.abspath(args.baseline_tree), args.reps))
        ours.append(child("census", ROOT, args.reps))
    om, oall = median_of(ours)
    bm, ball = median_of(base) if base else ({}, {})
    result = {"shape": {"w": W, "h": H, "block_size": BS, "D": MAXD, "view": "left"}, "reps": args.reps, "rounds": args.rounds,
              "census_tree_median_ms": om, "census_tree_rounds_ms": oall, "baseline_tree_median_ms": bm,
              "baseline_tree_rounds_ms": ball, "launch": ours[-1]["launch"], "match_kernel_build": MATCH_KERNEL_BUILD,
              "sgm_census": SGM_CENSUS, "sgm_sad": SGM_SAD}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_census.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
