"""The scheduling core of ws_batch_* (stereo_reconstruction_amd/csrc/ws_batch_core.h) is HIP-free: compiled here with
g++ -fsanitize=thread and driven by tests/cxx/batch_core_check.cpp with fake workers of uneven speed, a worker that
fails mid-queue, a failing wait, a throwing item, and the real band plan of a trainingH batch.  Host only."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_batch_core_under_thread_sanitizer(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the check"
    exe = str(tmp_path / "batch_core_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=thread", "-pthread", "-I", ROOT,
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "batch_core_check.cpp")])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stderr[-4000:]
    assert "batch core ok" in r.stdout


def test_batch_search_opencv_overload_compiles_against_the_stub():
    """wsamd::BatchSearch::run(params, cv::Mat pairs): a syntax-and-types check against tests/cxx/opencv_stub, NOT
    against OpenCV itself (there is none in this image)."""
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "tests", "cxx", "opencv_stub"), "-I", ROOT,
                           os.path.join(ROOT, "tests", "cxx", "batch_opencv_check.cpp")])
