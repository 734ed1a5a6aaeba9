"""The copy pool behind the staged host paths (stereo_reconstruction_amd/csrc/ws_copy_pool.h) is HIP-free: compiled here
with g++ -fsanitize=thread and driven by tests/cxx/copy_pool_check.cpp -- plain copies of random sizes, two threads
submitting at once, the three widening kinds (int16 -> float / double, float -> double) and a child forked while a copy
runs.  Host only."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_copy_pool_under_thread_sanitizer(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the check"
    exe = str(tmp_path / "copy_pool_check")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=thread", "-pthread", "-I", ROOT,
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "copy_pool_check.cpp")])
    # 6 threads per copy (5 helpers), whatever the host's core count
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", WS_COPY_THREADS="6")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "copy pool ok" in r.stdout
