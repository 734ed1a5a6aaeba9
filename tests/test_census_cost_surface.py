"""The census-transform cost's surface without a device: the library exports the transform's entry points and the Python
binding names the two costs, ws_validate / ws_validate_sgm accept them and make every refusal of the rules, ws_plan
reports the match kernel, ws_sgm_scratch_bytes switches the cost width at the bound, a batch with a census job is never
cut into row bands, and the C++ facade compiles and links."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ARG, GEOMETRY, UNSUPPORTED = -1, -2, -3
COSTS = ["census5x5", "census9x7"]


def images(w=40, h=30, w2=None, h2=None):
    return np.full((h, w, 3), 9, np.uint8), np.full((h2 or h, w2 or w, 3), 9, np.uint8)


def validate(wslib, p, L, R):
    return wslib.validate(p, L.shape, R.shape)


def test_symbols_and_constants(wslib):
    lib = wslib.load_library()
    for name in ("ws_census_transform_device", "ws_census_transform_host"):
        assert hasattr(lib, name), name
        assert name in wslib.EXPORTS, name
    assert (wslib.COST_CENSUS_5X5, wslib.COST_CENSUS_9X7) == (2, 3)
    assert wslib.make_params(wslib.VIEW_LEFT, cost="census5x5").cost == 2
    assert wslib.make_params(wslib.VIEW_LEFT, cost="census9x7").cost == 3
    assert wslib.make_params(wslib.VIEW_LEFT, cost=wslib.COST_CENSUS_9X7).cost == 3
    assert lib.ws_version() == 100
    assert callable(wslib.WindowSearch.census_transform) and callable(wslib.WindowSearch.census_transform_device)


def test_header_constants_and_params_layout(wslib, tmp_path):
    src = tmp_path / "ct_layout.c"
    src.write_text('#include <stdio.h>\n#include "include/ws_stereo.h"\n'
                   'int main(void) { printf("%d %d %zu %d\\n", WS_COST_CENSUS_5X5, WS_COST_CENSUS_9X7, sizeof(ws_params), WS_VERSION);\n'
                   "  return 0; }\n")
    exe = str(tmp_path / "ct_layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", ROOT, "-o", exe, str(src)])
    c5, c9, size, version = map(int, subprocess.check_output([exe]).split())
    assert (c5, c9, version) == (2, 3, 100)
    assert size == ctypes.sizeof(wslib._Params)


@pytest.mark.parametrize("cost", COSTS)
def test_accepted_in_both_views_with_subpixel(wslib, cost):
    L, R = images()
    for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT):
        for sub in (False, True):
            for bs in (1, 5, 63):
                p = wslib.make_params(view, bs, 0, 16, cost=cost, subpixel=sub)
                assert validate(wslib, p, L, R) == 0, (view, sub, bs)
                for paths in (4, 8):
                    assert wslib.validate_sgm(p, L, R, paths, 3, 20) == 0
    p = wslib.make_params(wslib.VIEW_RIGHT, 4, 2, 5000, cost=cost)     # an even block in the right view, a wide range
    assert validate(wslib, p, L, R) == 0


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("what,code", [
    ("smooth_left", UNSUPPORTED), ("smooth_right", UNSUPPORTED), ("smooth_zero_left", UNSUPPORTED),
    ("var_block_right", UNSUPPORTED), ("even_block_left", GEOMETRY), ("block_64", ARG), ("block_0", ARG),
    ("negative_min_right", GEOMETRY), ("right_taller_image", GEOMETRY), ("nan_smooth", ARG)])
def test_every_refusal(wslib, cost, what, code):
    L, R = images()
    view = wslib.VIEW_RIGHT if what.endswith("_right") else wslib.VIEW_LEFT
    p = wslib.make_params(view, 5, 0, 16, cost=cost)
    if what.startswith("smooth_zero"):
        p.smooth_factor = 0.0
    elif what.startswith("smooth"):
        p.smooth_factor = 0.5
    elif what == "var_block_right":
        p.var_block = 1
    elif what == "even_block_left":
        p.block_size = 4
    elif what == "block_64":
        p.block_size = 64
    elif what == "block_0":
        p.block_size = 0
    elif what == "negative_min_right":
        p.min_disparity = -2
    elif what == "right_taller_image":
        p = wslib.make_params(wslib.VIEW_RIGHT, 5, 0, 16, cost=cost)
        L, R = images(40, 30, h2=33)
    elif what == "nan_smooth":
        p.smooth_factor = float("nan")
    assert validate(wslib, p, L, R) == code, what
    assert wslib.validate_sgm(p, L, R, 8, 1, 2) == code, what


def test_other_cost_values_stay_refused_and_linear_ignores_the_cost(wslib):
    L, R = images()
    for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT):
        for cost in (4, 5, -1, 62):
            p = wslib.make_params(view, 5, 0, 16)
            p.cost = cost
            assert validate(wslib, p, L, R) == ARG, cost
            assert wslib.validate_sgm(p, L, R) == ARG, cost
    # var_block in the LEFT view is ignored by the reference and stays accepted
    p = wslib.make_params(wslib.VIEW_LEFT, 5, 0, 16, cost="census9x7", var_block=True)
    assert validate(wslib, p, L, R) == 0
    for cost in (2, 3):
        p = wslib.make_params(wslib.VIEW_LINEAR)
        p.cost = cost
        p.smooth_factor = 0.5
        assert validate(wslib, p, L, R) == 0


@pytest.mark.parametrize("cost", COSTS)
def test_plan_reports_the_match_kernel(wslib, cost):
    for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT):
        info = wslib.plan(wslib.make_params(view, 7, 0, 64, cost=cost), (375, 450), (375, 450))
        assert info["marching"] == 0 and info["kernel_kind"] == 2
        assert info["threads"] == 256 and info["tile_cols"] == 64 and info["strip_rows"] == 32
        assert info["tiles"] == (450 + 63) // 64 and info["strips"] == (375 + 31) // 32
        assert 0 < info["lds_bytes"] <= 65536
        assert info["d_chunks"] == (64 + 61) // 62 if view == wslib.VIEW_LEFT else info["d_chunks"] >= 1
    assert wslib.plan(wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64, cost="sad"), (375, 450), (375, 450))["kernel_kind"] in (0, 1)


def test_sgm_scratch_switches_the_cost_width_at_the_bound(wslib):
    """16-bit costs while bits * bs^2 <= 65535: 9x7 up to block size 31, 5x5 up to 51; the descriptor planes are counted."""
    w, h, D = 200, 90, 32
    L, R = images(w, h)

    def cost_plane_bytes(cost, bs):
        # (the left view keeps min(D, w - 1 - 2 half) disparities: D here)
        total = wslib.sgm_scratch_bytes(wslib.make_params(wslib.VIEW_LEFT, bs, 0, D, cost=cost), L, R, 8, 3, 20)
        planes = 2 * w * h * (4 if cost == "census5x5" else 8)
        assert total >= w * h * 4 + w * h * D * (2 + 4) + planes
        return total

    vol = w * h * D
    for cost, below, above in (("census9x7", 31, 33), ("census5x5", 51, 53)):
        a, b = cost_plane_bytes(cost, below), cost_plane_bytes(cost, above)
        assert b - a == 2 * vol, (cost, a, b)                     # 16 -> 32 bits per cost, nothing else changes
        assert cost_plane_bytes(cost, below - 2) == a
    # the descriptor planes: a census call holds them on top of what the same call with SAD holds at equal widths
    sad = wslib.sgm_scratch_bytes(wslib.make_params(wslib.VIEW_LEFT, 5, 0, D, cost="sad"), L, R, 8, 3, 20)
    up = lambda n: (n + 255) & ~255
    assert cost_plane_bytes("census5x5", 5) - sad == 2 * up(w * h * 4)
    assert cost_plane_bytes("census9x7", 5) - sad == 2 * up(w * h * 8)


def test_a_batch_with_a_census_job_is_not_banded(wslib):
    from stereo_reconstruction_amd.sharding import can_band
    shapes = [(600, 500)] * 3
    sad = wslib.make_params(wslib.VIEW_LEFT, 7, 0, 64, cost="sad")
    items, banded = wslib.batch_plan(sad, shapes, 4, bands=True, min_rows=64)
    assert banded and len(items) > 3
    assert can_band(sad.view, sad.smooth_factor, sad.var_block, sad.cost, 600, 600)
    for cost in COSTS:
        for view in (wslib.VIEW_LEFT, wslib.VIEW_RIGHT):
            p = wslib.make_params(view, 7, 0, 64, cost=cost)
            assert not can_band(p.view, p.smooth_factor, p.var_block, p.cost, 600, 600)
            items, banded = wslib.batch_plan(p, shapes, 4, bands=True, min_rows=64)
            assert not banded
            assert sorted((j, y0, y1) for j, y0, y1, _ in items) == [(j, 0, 600) for j in range(3)]
            # one census job among SAD jobs keeps the whole batch in whole pairs
            items, banded = wslib.batch_plan([sad, p, sad], shapes, 4, bands=True, min_rows=64)
            assert not banded and len(items) == 3


def test_transform_argument_checks_need_no_device(wslib):
    lib = wslib.load_library()
    img = wslib._shape_image((8, 9))
    out = (ctypes.c_uint64 * 72)()
    assert lib.ws_census_transform_host(None, ctypes.byref(img), 2, out, 9) == ARG
    assert lib.ws_census_transform_device(None, ctypes.byref(img), 3, out, 9, None) == ARG


def test_cxx_facade_compiles_and_links(wslib, tmp_path):
    """tests/cxx/census_driver.cpp: BlockSearch with a census cost and wsamd::censusTransform, as a caller writes them."""
    exe = str(tmp_path / "census_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cxx", "census_driver.cpp"),
                           "-L", os.path.join(ROOT, "stereo_reconstruction_amd"), "-lws_stereo",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_reconstruction_amd")])
    assert os.path.exists(exe)
