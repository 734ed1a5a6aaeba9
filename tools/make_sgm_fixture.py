"""Write tests/golden/teddyH_sgm.json: the SHA-1 of whole SGM maps of the Teddy-H pair, computed by the NumPy
restatement tests/sgm_ref.py (too slow to run inside the GPU suite).  CPU only.

    python tools/make_sgm_fixture.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sgm_ref  # noqa: E402

# (view, cost, block_size, paths, p1, p2, subpixel): the left view at the issue's quality settings, the right view in
# SSD with sub-pixel refinement
CASES = [("left", "sad", 5, 8, 600, 2400, False), ("right", "ssd", 5, 4, 20000, 80000, True)]


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "teddyH_pair.npz"))
    L, R, nd = z["left"], z["right"], int(z["ndisp"])
    out = []
    for view, cost, bs, paths, p1, p2, sub in CASES:
        m = sgm_ref.sgm_np(L, R, view, bs, 0, nd, cost, paths, p1, p2, subpixel=sub).astype(np.float32)
        out.append({"view": view, "cost": cost, "block_size": bs, "min_disparity": 0, "max_disparity": nd, "paths": paths,
                    "p1": p1, "p2": p2, "subpixel": sub, "sha1": hashlib.sha1(np.ascontiguousarray(m).tobytes()).hexdigest()})
        print(out[-1], flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "teddyH_sgm.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
