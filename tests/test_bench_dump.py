"""bench.py --dump-outputs: the maps the last timed step computed, written so that two builds run with the same
arguments can be compared file for file (whole maps of a seeded choice of pairs + a seeded sample of every pair,
float32, at most 64 MB).  The writer is checked on host tensors here; the GPU test runs bench.py itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_bench_launcher import json_line, run_bench


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_whole_maps_and_a_sample_within_the_budget(tmp_path):
    import torch
    bench = _bench_module()
    rng = np.random.default_rng(5)
    # config 2's map shape, more pairs than whole maps fit: the budget and the cap on whole maps both bind
    outs = [torch.from_numpy((1000 * k + rng.integers(0, 256, size=(1000, 1500))).astype(np.float32)) for k in range(12)]
    files = bench.dump_outputs(str(tmp_path / "a"), outs)
    assert _dir_bytes(tmp_path / "a") <= bench.DUMP_BYTES
    assert sorted(os.listdir(tmp_path / "a")) == sorted(files)
    whole = [f for f in files if f.startswith("disparity_pair")]
    assert "disparity_pair0.npy" in whole and len(whole) == bench.DUMP_WHOLE_MAPS
    for f in whole:
        got = np.load(tmp_path / "a" / f)
        assert got.dtype == np.float32 and np.array_equal(got, outs[int(f[len("disparity_pair"):-4])].numpy())
    sample = np.load(tmp_path / "a" / "disparity_sample.npy")
    assert sample.dtype == np.float32 and sample.ndim == 1 and sample.size % len(outs) == 0
    per = sample.size // len(outs)
    for k in range(len(outs)):                          # every pair contributes its own values, in batch order
        assert ((sample[k * per:(k + 1) * per] // 1000) == k).all()
    # the same maps give the same files
    bench.dump_outputs(str(tmp_path / "b"), outs)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_dump_of_maps_larger_than_the_budget_keeps_to_it(tmp_path):
    import torch
    bench = _bench_module()
    outs = [torch.full((2160, 3840), float(k), dtype=torch.float32) for k in range(4)]   # config 5: 33 MB a map
    files = bench.dump_outputs(str(tmp_path), outs)
    assert _dir_bytes(tmp_path) <= bench.DUMP_BYTES
    assert "disparity_pair0.npy" in files and len(files) == 2
    sample = np.load(tmp_path / "disparity_sample.npy")
    assert np.array_equal(sample, np.repeat(np.arange(4, dtype=np.float32), sample.size // 4))


def test_steps_must_be_positive_and_the_rehearsal_has_nothing_to_dump(tmp_path):
    p = run_bench("--steps", "0")
    assert p.returncode != 0 and "--steps" in p.stderr
    p = run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "d"))
    assert p.returncode != 0 and "--dump-outputs" in p.stderr


@pytest.mark.gpu
def test_bench_dump_is_the_timed_path_s_output(tmp_path, oracle):
    """Config 1 with a batch of 4: pair k is pair 0's scene rolled down by 37 k rows (bench.py); every whole map dumped
    is the oracle's, and a second run with another number of steps dumps the same files."""
    from stereo_reconstruction_amd.synthetic import make_pair
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "WS_BENCH_REHEARSE")}
    runs = []
    for steps in ("3", "1"):
        d = str(tmp_path / ("s" + steps))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "config1", "--pairs-per-step", "4",
                            "--steps", steps, "--warmup", "1", "--no-extras", "--no-cpu-baseline", "--dump-outputs", d],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out = json_line(p.stdout)
        assert out["steps"] == int(steps) and out["ms_per_step"] > 0
        assert sorted(out["dump_outputs"]["files"]) == sorted(os.listdir(d))
        runs.append(d)
    files = sorted(os.listdir(runs[0]))
    assert files == sorted(os.listdir(runs[1])) and len(files) == 5          # 4 whole maps + the sample
    for f in files:
        assert np.array_equal(np.load(os.path.join(runs[0], f)), np.load(os.path.join(runs[1], f))), f
    left, right, _ = make_pair(450, 375, 64, 1)
    for k in (0, 3):
        want = oracle.block_left(np.roll(left, 37 * k, 0), np.roll(right, 37 * k, 0), 5, 0, 64, cost="sad", threads=8)
        got = np.load(os.path.join(runs[0], "disparity_pair%d.npy" % k))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), k
