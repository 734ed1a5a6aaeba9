"""The mesh text formatter the kernels use (stereo_reconstruction_amd/csrc/ws_text.h), built with g++ on the host and
compared byte for byte with the C library's "%g" / "%llu" (tests/cxx/mesh_text_check.cpp): whole binades around the
%f / %e switch, +-4 ulps of every power of ten, every 7-digit tie, the special values and 10^8 random bit patterns."""
import os
import subprocess

from conftest import ROOT


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _build(tmp_path):
    exe = str(tmp_path / "mesh_text_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "mesh_text_check.cpp")])
    return exe


def test_g_format_equals_printf_on_every_class_of_float(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, str(_threads()), "100000000"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok:")


def test_the_issue_cases_by_name(tmp_path):
    """The rounding cases named for the formatter, through a tiny host program."""
    src = tmp_path / "cases.cpp"
    src.write_text('#include "stereo_reconstruction_amd/csrc/ws_text.h"\n#include <stdio.h>\n#include <math.h>\n'
                   'int main() { const float v[] = {1234565.f, 123456.5f, 999999.5f, 1e-05f, 0.0001f, -0.0f, INFINITY,'
                   ' -INFINITY, NAN, -NAN, 1e-45f, 3.40282347e+38f};\n'
                   '  for (float f : v) { char b[16]; int n = wsamd::text::g_format(f, b); printf("%.*s\\n", n, b); }'
                   '  char b[24]; int n = wsamd::text::u_format((unsigned long long)4294967295u, b); printf("%.*s\\n", n, b); }\n')
    exe = str(tmp_path / "cases")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True).split("\n")
    assert out[:13] == ["1.23456e+06", "123456", "1e+06", "1e-05", "0.0001", "-0", "inf", "-inf", "nan", "-nan",
                        "1.4013e-45", "3.40282e+38", "4294967295"]
