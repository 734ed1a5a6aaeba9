"""BASELINE config 4's batch through the host-buffer entry points: the 15 trainingH-shaped pairs (7x7 SSD, D 256, left
view, float32 maps) through WindowSearch.search_many on one context, or through BatchSearch with a list of workers
(whole pairs or row bands).  One configuration per process, so that each runs under a time limit of its own:

    python tools/time_batch.py --mode many
    python tools/time_batch.py --mode batch --workers 0,0 [--whole]
    python tools/time_batch.py --mode batch --workers all

Prints one line: median / min wall ms per batch over --reps calls after --warmup, and Mdisp/s (hypotheses per second);
with --append FILE the line is also appended there.  Every map is checked against the one-context maps once."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_reconstruction_amd as ws  # noqa: E402
from stereo_reconstruction_amd.synthetic import TRAINING_H, make_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["many", "batch"], required=True)
    ap.add_argument("--workers", default="0", help="comma-separated device per worker, or 'all'")
    ap.add_argument("--whole", action="store_true", help="whole pairs only (no row bands)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--append", default="")
    a = ap.parse_args()
    pairs = [make_pair(w, h, 256, 500 + k)[:2] for k, (_, w, h, _) in enumerate(TRAINING_H)]
    hyps = float(sum(w * h * 256 for _, w, h, _ in TRAINING_H))
    p = ws.make_params(ws.VIEW_LEFT, 7, 0, 256, 1.0, "ssd")
    with ws.WindowSearch(0) as ctx:
        want = ctx.search_many(p, pairs, dtype=np.float32)
        if a.mode == "many":
            label = "search_many, one context"
            run = lambda: ctx.search_many(p, pairs, dtype=np.float32)  # noqa: E731
            times = measure(run, want, a)
        else:
            devices = None if a.workers == "all" else [int(d) for d in a.workers.split(",")]
            with ws.BatchSearch(devices) as b:
                items, banded = b.plan(p, pairs, bands=not a.whole)
                label = "BatchSearch workers=%s %s (%d items)" % (b.workers, "bands" if banded else "whole pairs", len(items))
                run = lambda: b.search(p, pairs, dtype=np.float32, bands=not a.whole)  # noqa: E731
                times = measure(run, want, a)
    med, lo = float(np.median(times)), float(np.min(times))
    line = "%-62s median %8.2f ms  min %8.2f ms  %9.0f Mdisp/s (median)" % (label, med, lo, hyps / (med * 1e-3) / 1e6)
    print(line, flush=True)
    if a.append:
        with open(a.append, "a") as f:
            f.write(line + "\n")


def measure(run, want, a):
    got = run()
    for g, w in zip(got, want):
        if not np.array_equal(g, w):
            raise SystemExit("a map differs from the one-context map")
    for _ in range(a.warmup):
        run()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


if __name__ == "__main__":
    main()
