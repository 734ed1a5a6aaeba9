"""Wall time of the mesh writer at 900x750 and 3840x2160 (or --sizes WxH,...): the host pair ws_back_project +
ws_write_mesh_off against ws_reconstruction_host (vertices and text built on the device, only the text comes down),
and the floor under both -- writing the same bytes from host memory to a file in the same directory.

    python tools/time_mesh.py [--reps 3] [--dir DIR] [--sizes 900x750,3840x2160]

The files go to DIR (default: a fresh directory under the current one, removed at the end).

With WS_HOST_TRACE=1 each device call also prints its split on stderr (us since the call's text phase began: `sized` =
count + scan kernels done, chunk_wait_total = waiting for the write kernel and the chunk downloads, fwrite_total = time
in fwrite).  The kernels themselves: rocprofv3 --kernel-trace --stats -- python tools/time_mesh.py --reps 1.
Prints one JSON line per size."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_reconstruction_amd as ws  # noqa: E402


def scene(w, h, seed=5):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    disp = np.rint(40 + 20 * np.sin(xs / 97.0) * np.cos(ys / 61.0) + rng.integers(-1, 2, size=(h, w))).astype(np.float32)
    disp[rng.random((h, w)) < 0.05] = 0
    bgr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    K = np.array([[3000, 0, w / 2], [0, 3000, h / 2], [0, 0, 1]], dtype=np.float32)
    return disp, bgr, K


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t) * 1e3, float(np.median(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the mesh files are written (default: a fresh directory under the current one)")
    ap.add_argument("--sizes", default="900x750,3840x2160")
    a = ap.parse_args()
    own_dir = a.dir is None
    out_dir = tempfile.mkdtemp(prefix="time_mesh_", dir=os.getcwd()) if own_dir else a.dir
    os.makedirs(out_dir, exist_ok=True)
    try:
        run(a, out_dir)
    finally:
        if own_dir:
            shutil.rmtree(out_dir, ignore_errors=True)


def run(a, out_dir):
    host_p, dev_p, raw_p = (os.path.join(out_dir, n) for n in ("time_mesh_host.off", "time_mesh_device.off", "time_mesh_raw.bin"))
    with ws.WindowSearch(0) as ctx:
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            disp, bgr, K = scene(w, h)
            depth = ctx.convert_disparity_to_depth(disp, 3000.0, 0.1)
            thr = 0.05

            def host_pair():
                pos, col = ctx.back_project(depth, K, bgr)
                ws.write_mesh_off(host_p, pos, col, thr)

            def device_call():
                ctx.reconstruction(depth, K, bgr, thr, dev_p)

            dev = best(device_call, a.reps)
            host = best(host_pair, a.reps)
            with open(host_p, "rb") as f:
                text = f.read()
            with open(dev_p, "rb") as f:
                same = f.read() == text

            def raw_write():
                with open(raw_p, "wb") as f:
                    f.write(text)

            floor = best(raw_write, a.reps)
            print(json.dumps({"size": size, "bytes": len(text), "identical": same,
                              "host_pair_ms": [round(v, 2) for v in host], "reconstruction_host_ms": [round(v, 2) for v in dev],
                              "file_write_floor_ms": [round(v, 2) for v in floor], "speedup_min": round(host[0] / dev[0], 1)}),
                  flush=True)
    for p in (host_p, dev_p, raw_p):
        if os.path.exists(p):
            os.remove(p)


if __name__ == "__main__":
    main()
