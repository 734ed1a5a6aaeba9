"""The left-right check's surface without a device: the library exports its entry points, ws_lr_params has the header's
layout in the Python binding, the C++ facade's BlockSearch::computeDisparityMapsChecked compiles and links, and the
arguments are refused before any device is touched."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

LR_SYMBOLS = ["ws_lr_check_device", "ws_search_lr_host", "ws_search_lr_device", "ws_last_lr_counts"]


def test_library_exports_the_lr_entry_points(wslib):
    lib = wslib.load_library()
    for name in LR_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in wslib.EXPORTS, name
    assert lib.ws_version() == 100


def test_lr_params_layout_matches_the_header(wslib, tmp_path):
    src = tmp_path / "lr_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "include/ws_stereo.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %d %d\\n\", sizeof(ws_lr_params), _Alignof(ws_lr_params),\n"
                   "  offsetof(ws_lr_params, max_diff), offsetof(ws_lr_params, fill), WS_LR_FILL_NONE, WS_LR_FILL_BACKGROUND);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "lr_layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", ROOT, "-o", exe, str(src)])
    size, align, off_max, off_fill, none, background = map(int, subprocess.check_output([exe]).split())
    P = wslib._LrParams
    assert (size, align) == (ctypes.sizeof(P), ctypes.alignment(P))
    assert (off_max, off_fill) == (P.max_diff.offset, P.fill.offset)
    assert P.max_diff.size == ctypes.sizeof(ctypes.c_float) and P.fill.size == ctypes.sizeof(ctypes.c_int)
    assert (none, background) == (wslib.LR_FILL_NONE, wslib.LR_FILL_BACKGROUND)
    lr = wslib.lr_params(2.5, fill=True)
    assert (lr.max_diff, lr.fill) == (2.5, background)


def test_cxx_facade_checked_maps_compile_and_link(wslib, tmp_path):
    """wsamd::BlockSearch::computeDisparityMapsChecked, as a caller of the facade writes it (tests/cxx/lr_driver.cpp)."""
    exe = str(tmp_path / "lr_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "lr_driver.cpp"),
           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")]
    subprocess.check_call(cmd)
    assert os.path.exists(exe)


def test_lr_calls_refuse_a_missing_context(wslib):
    lib = wslib.load_library()
    counts = (ctypes.c_ulonglong * 2)()
    lr = wslib.lr_params(1.0)
    assert lib.ws_last_lr_counts(None, counts) == -1
    assert lib.ws_lr_check_device(None, None, 1, 1, 1, None, 1, 1, 1, ctypes.byref(lr), None, 1, None, 1, None) == -1
    assert lib.ws_search_lr_host(None, None, None, None, ctypes.byref(lr), None, 1, None, 1, 0) == -1
    assert lib.ws_search_lr_device(None, None, None, None, ctypes.byref(lr), None, 1, None, 1, None) == -1


@pytest.mark.parametrize("name", ["search_lr", "search_lr_device", "lr_check_device", "last_lr_counts"])
def test_python_surface_has_the_lr_methods(wslib, name):
    assert callable(getattr(wslib.WindowSearch, name))
    assert callable(wslib.BlockSearch.computeDisparityMapsChecked)
