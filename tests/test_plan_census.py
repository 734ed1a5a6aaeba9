"""The marching planner plans what it planned when tests/golden/plan_census.json was recorded: tools/plan_census.py's
grid (both views, both costs, 11 block sizes, 11 image sizes, 11 disparity ranges: 5 324 plans) at num_cus = 256, one
sha1 per (view, cost, block size) group.  The digests are recomputed in a child process that sees no HIP device, so the
planner's occupancy question takes its rule of thumb on every machine and like is compared with like."""
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT

KNOBS = ("WS_MARCH_ND", "WS_MARCH_HALO", "WS_MARCH_HALO_SSD", "WS_PLAN_SLOTS", "WS_PLAN_THREADS", "WS_MAX_CHUNKS",
         "WS_MARCH_MFMA", "WS_STEREO_LIB")


def test_plans_match_the_recorded_census(wslib, tmp_path):
    with open(os.path.join(GOLDEN, "plan_census.json")) as f:
        want = json.load(f)
    out = str(tmp_path / "census.json")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_census.py"), "--no-device", "--num-cus",
                           str(want["num_cus"]), "--json", out], env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    with open(out) as f:
        got = json.load(f)
    assert got["devices"] == 0, "the child process still sees a HIP device"
    assert got["plans"] == want["plans"] == 5324
    assert sorted(got["groups"]) == sorted(want["groups"])
    differ = [g for g in want["groups"] if got["groups"][g] != want["groups"][g]]
    assert not differ, "plans changed in the groups %s (tools/plan_census.py --dump shows each plan)" % differ
    assert got["all"] == want["all"]
