"""Census of the marching planner: ws.plan over a grid of searches, one sha1 per (view, cost, block size) group and one
over everything.  Two builds plan alike exactly when their digests are equal.  No device is needed: without one the
planner's occupancy question falls back to its rule of thumb, with one it asks the runtime (so compare like with like).

    python tools/plan_census.py                        # digests at num_cus = 256
    python tools/plan_census.py --num-cus 0            # ... at the CU count of device 0
    python tools/plan_census.py --no-device            # hide every HIP device from this process first
    python tools/plan_census.py --json out.json        # also write {"groups": {...}, "all": ..., ...}
    python tools/plan_census.py --dump plans.txt       # one line per plan
    python tools/plan_census.py --against plans.txt    # count the plans that differ from a dump of another build

tests/golden/plan_census.json holds the device-less digests at num_cus = 256 (tests/test_plan_census.py).
"""
import argparse
import hashlib
import json
import os
import sys
import time

VIEWS = (("left", 0), ("right", 1))
COSTS = ("ssd", "sad")
BLOCK_SIZES = (3, 5, 6, 7, 8, 9, 11, 13, 15, 17, 19)
SIZES = ((40, 30), (97, 61), (160, 120), (255, 129), (320, 96), (390, 198), (700, 300), (1500, 1000), (2964, 1988),
         (3840, 2160), (6000, 500))  # width x height
MAX_DISPARITIES = (1, 7, 16, 64, 128, 200, 256, 257, 512, 1024, 3000)


def census(ws, num_cus):
    """{(view, cost, block size): [one line per plan]} over the whole grid, in a fixed order."""
    groups = {}
    for vname, view in VIEWS:
        for cost in COSTS:
            for bs in BLOCK_SIZES:
                lines = groups.setdefault("%s/%s/bs%d" % (vname, cost, bs), [])
                for w, h in SIZES:
                    for maxd in MAX_DISPARITIES:
                        p = ws.make_params(view, bs, 0, maxd, 1.0, cost)
                        try:
                            info = ws.plan(p, (h, w), (h, w), num_cus)
                            what = " ".join("%s=%d" % kv for kv in info.items())
                        except ws.WsError as e:  # (the left view refuses even block sizes: part of the record)
                            what = "error=%d" % e.code
                        lines.append("%dx%d D=%d: %s" % (w, h, maxd, what))
    return groups


def digests(groups):
    per = {k: hashlib.sha1("\n".join(v).encode()).hexdigest() for k, v in groups.items()}
    whole = hashlib.sha1("\n".join(k + " " + line for k, v in groups.items() for line in v).encode()).hexdigest()
    return per, whole


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-cus", type=int, default=256, help="the CU count to plan for; 0 = device 0's own")
    ap.add_argument("--no-device", action="store_true", help="hide every HIP device from this process")
    ap.add_argument("--json", help="write the digests here")
    ap.add_argument("--dump", help="write one line per plan here")
    ap.add_argument("--against", help="count the plans that differ from this dump")
    args = ap.parse_args()
    if args.no_device:
        os.environ["HIP_VISIBLE_DEVICES"] = os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import stereo_reconstruction_amd as ws

    devices = ws.device_count()
    num_cus = args.num_cus
    if num_cus <= 0:
        import torch
        num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    t0 = time.time()
    groups = census(ws, num_cus)
    per, whole = digests(groups)
    n = sum(len(v) for v in groups.values())
    for k, d in per.items():
        print("%-20s %s" % (k, d))
    print("%-20s %s" % ("all", whole))
    print("%d plans in %.1f s, num_cus = %d, %d HIP device(s) visible" % (n, time.time() - t0, num_cus, devices))
    flat = [k + " " + line for k, v in groups.items() for line in v]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"num_cus": num_cus, "devices": devices, "plans": n, "all": whole, "groups": per}, f, indent=1)
            f.write("\n")
    if args.dump:
        with open(args.dump, "w") as f:
            f.write("\n".join(flat) + "\n")
    if args.against:
        with open(args.against) as f:
            other = f.read().splitlines()
        differ = [(a, b) for a, b in zip(flat, other) if a != b]
        print("%d of %d plans differ from %s" % (len(differ) + abs(len(flat) - len(other)), n, args.against))
        for a, b in differ[:10]:
            print("  here:  %s\n  there: %s" % (a, b))


if __name__ == "__main__":
    main()
