"""The speckle filter's surface without a device: the library exports its entry points, ws_speckle_params has the header's
layout in the Python binding, the C++ facade's wsamd::filterSpeckles compiles and links, and every refusal of rule 6 in
include/ws_stereo.h is returned before any device work -- the arguments are checked before the context is."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SPECKLE_SYMBOLS = ["ws_filter_speckles_device", "ws_filter_speckles_host", "ws_last_speckle_counts"]
WS_ERR_ARG = -1


def test_library_exports_the_speckle_entry_points(wslib):
    lib = wslib.load_library()
    for name in SPECKLE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in wslib.EXPORTS, name
    assert lib.ws_version() == 100


def test_speckle_params_layout_matches_the_header(wslib, tmp_path):
    src = tmp_path / "speckle_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "include/ws_stereo.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu\\n\", sizeof(ws_speckle_params), _Alignof(ws_speckle_params),\n"
                   "  offsetof(ws_speckle_params, new_val), offsetof(ws_speckle_params, max_speckle_size),\n"
                   "  offsetof(ws_speckle_params, max_diff));\n  return 0; }\n")
    exe = str(tmp_path / "speckle_layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", ROOT, "-o", exe, str(src)])
    size, align, off_nv, off_size, off_diff = map(int, subprocess.check_output([exe]).split())
    P = wslib._SpeckleParams
    assert (size, align) == (ctypes.sizeof(P), ctypes.alignment(P))
    assert (off_nv, off_size, off_diff) == (P.new_val.offset, P.max_speckle_size.offset, P.max_diff.offset)
    assert P.new_val.size == P.max_diff.size == ctypes.sizeof(ctypes.c_float)
    assert P.max_speckle_size.size == ctypes.sizeof(ctypes.c_int)
    sp = wslib.speckle_params(-1.5, 42, 2.25)
    assert (sp.new_val, sp.max_speckle_size, sp.max_diff) == (-1.5, 42, 2.25)
    sp = wslib.speckle_params()
    assert (sp.new_val, sp.max_speckle_size, sp.max_diff) == (0.0, 100, 1.0)


def test_cxx_facade_filter_speckles_compiles_and_links(wslib, tmp_path):
    """wsamd::filterSpeckles, as a caller of the facade writes it (tests/cxx/speckle_driver.cpp)."""
    exe = str(tmp_path / "speckle_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "speckle_driver.cpp"),
           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")]
    subprocess.check_call(cmd)
    assert os.path.exists(exe)


def _call(lib, which, ptr, w, h, stride, sp):
    if which == "device":
        return lib.ws_filter_speckles_device(None, ptr, w, h, stride, sp, None)
    return lib.ws_filter_speckles_host(None, ptr, w, h, stride, sp)


REFUSALS = [  # (what, params or None, w, h, stride, map present, word in the message)
    ("new_val NaN", (float("nan"), 10, 1.0), 8, 4, 8, True, "new_val"),
    ("max_diff NaN", (0.0, 10, float("nan")), 8, 4, 8, True, "max_diff"),
    ("max_diff negative", (0.0, 10, -0.5), 8, 4, 8, True, "max_diff"),
    ("max_speckle_size negative", (0.0, -1, 1.0), 8, 4, 8, True, "max_speckle_size"),
    ("null params", None, 8, 4, 8, True, "params"),
    ("null map", (0.0, 10, 1.0), 8, 4, 8, False, "map"),
    ("w < 1", (0.0, 10, 1.0), 0, 4, 8, True, "size"),
    ("h < 1", (0.0, 10, 1.0), 8, 0, 8, True, "size"),
    ("stride < w", (0.0, 10, 1.0), 8, 4, 7, True, "stride"),
    ("w * h >= 2^31", (0.0, 10, 1.0), 65536, 32768, 65536, True, "2^31"),
]


@pytest.mark.parametrize("which", ["device", "host"])
@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_is_named_before_the_context_is_looked_at(wslib, which, case):
    """With a null context a refusal of rule 6 is reported as that refusal (ws_last_error(NULL)), so it was decided
    before the context -- let alone a device -- was touched."""
    lib = wslib.load_library()
    what, params, w, h, stride, has_map, word = REFUSALS[case]
    m = np.zeros(64, np.float32)
    sp = ctypes.byref(wslib.speckle_params(*params)) if params else None
    assert _call(lib, which, m.ctypes.data if has_map else None, w, h, stride, sp) == WS_ERR_ARG, what
    assert word in lib.ws_last_error(None).decode(), (what, lib.ws_last_error(None))


@pytest.mark.parametrize("which", ["device", "host"])
def test_valid_arguments_reach_the_context_check(wslib, which):
    lib = wslib.load_library()
    m = np.zeros(64, np.float32)
    for params in ((0.0, 0, 0.0), (-0.0, 10, float("inf")), (float("inf"), 2**31 - 1, 3.0)):
        sp = wslib.speckle_params(*params)
        assert _call(lib, which, m.ctypes.data, 8, 4, 9, ctypes.byref(sp)) == WS_ERR_ARG
        assert "null context" in lib.ws_last_error(None).decode()
    counts = (ctypes.c_ulonglong * 2)()
    assert lib.ws_last_speckle_counts(None, counts) == WS_ERR_ARG


@pytest.mark.parametrize("name", ["filter_speckles", "filter_speckles_device", "last_speckle_counts"])
def test_python_surface_has_the_speckle_methods(wslib, name):
    assert callable(getattr(wslib.WindowSearch, name))
