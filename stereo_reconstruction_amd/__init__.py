"""MI355X-native WindowSearch: Python binding of the C-ABI (include/ws_stereo.h).

The product is the shared library `libws_stereo.so` (hand-written gfx950 HIP kernels
behind a C-ABI) and the C++ facade in `host/window_search.hpp`.  This module is the
thin ctypes layer the tests and bench.py call through; it mirrors the reference's
class surface:

    BlockSearch(left, right, blockSize, minDisparity, maxDisparity)   BlockSearch.h:11-15
        .computeDisparityMapLeft(smoothFactor)                         BlockSearch.h:28
        .computeDisparityMapRight(smoothFactor, varBlock, thres)       BlockSearch.h:37
    LinearSearch(left, right).computeDisparityMap(smoothFactor)        LinearSearch.h:13-19
    ImageRectifier(left, right, H_, Hp_)                                rectification.cpp:66-88, :432-505
        .computeDisparityMapLeft/Right(...), .getRectifiedLeft/Right(), .getDisparityMapLeft/Right()

There is no CPU fallback: if the library is missing or no HIP device answers, the calls
raise.  The CPU oracle under oracle/ is test infrastructure and is never imported here.
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np

from . import build as _build

__all__ = ["WindowSearch", "BatchSearch", "BlockSearch", "LinearSearch", "ImageRectifier", "WsError", "load_library", "rectified_size",
           "read_pfm", "write_pfm", "read_ppm", "write_ppm", "write_mesh_off", "read_calib", "evaldisp", "VIEW_LEFT", "VIEW_RIGHT",
           "VIEW_LINEAR", "COST_SSD", "COST_SAD", "COST_CENSUS_5X5", "COST_CENSUS_9X7"]

VIEW_LEFT, VIEW_RIGHT, VIEW_LINEAR = 0, 1, 2
COST_SSD, COST_SAD = 0, 1
COST_CENSUS_5X5, COST_CENSUS_9X7 = 2, 3  # the Hamming distance of census-transform descriptors (rules in include/ws_stereo.h)
OUT_F32, OUT_F64 = 0, 1
_COST = {"ssd": COST_SSD, "sad": COST_SAD, "census5x5": COST_CENSUS_5X5, "census9x7": COST_CENSUS_9X7,
         COST_SSD: COST_SSD, COST_SAD: COST_SAD, COST_CENSUS_5X5: COST_CENSUS_5X5, COST_CENSUS_9X7: COST_CENSUS_9X7}

ERRORS = {-1: "WS_ERR_ARG", -2: "WS_ERR_GEOMETRY", -3: "WS_ERR_UNSUPPORTED", -4: "WS_ERR_HIP",
          -5: "WS_ERR_IO", -6: "WS_ERR_NOMEM"}

# every symbol include/ws_stereo.h declares (tests check the library exports all of them)
EXPORTS = ["ws_version", "ws_params_default", "ws_create", "ws_destroy", "ws_last_error",
           "ws_device_count", "ws_validate", "ws_plan", "ws_search_host", "ws_search_device", "ws_enqueue_host", "ws_wait", "ws_warp_nearest_host",
           "ws_warp_nearest_device", "ws_remove_disparity_outliers", "ws_convert_disparity_to_depth",
           "ws_back_project", "ws_write_mesh_off", "ws_write_mesh_off_device", "ws_reconstruction_host",
           "ws_timer_begin", "ws_timer_end", "ws_set_profiling", "ws_last_kernel_ms",
           "ws_last_launch_info", "ws_last_max_block", "ws_set_tuning", "ws_set_host_bands", "ws_last_host_paths", "ws_last_wire_format", "ws_last_outliers_path", "ws_last_outliers_forms", "ws_device_status",
           "ws_pfm_read", "ws_pfm_write", "ws_free", "ws_ppm_read", "ws_ppm_write", "ws_calib_read", "ws_evaldisp",
           "ws_rectified_size", "ws_rectify_device", "ws_search_unrectified_host",
           "ws_batch_create", "ws_batch_destroy", "ws_batch_last_error", "ws_batch_workers", "ws_batch_plan",
           "ws_batch_search_host", "ws_lr_check_device", "ws_search_lr_host", "ws_search_lr_device", "ws_last_lr_counts",
           "ws_filter_speckles_device", "ws_filter_speckles_host", "ws_last_speckle_counts",
           "ws_validate_sgm", "ws_sgm_scratch_bytes", "ws_search_sgm_device", "ws_search_sgm_host",
           "ws_validate_unique", "ws_unique_scratch_bytes", "ws_search_unique_device", "ws_search_unique_host",
           "ws_last_unique_counts", "ws_validate_pair", "ws_search_pair_device", "ws_search_pair_host",
           "ws_census_transform_device", "ws_census_transform_host"]
JOB_NOT_RUN = 1  # ws_job.status of a job its worker never reached (WS_JOB_NOT_RUN)


class WsError(RuntimeError):
    def __init__(self, code, message=""):
        self.code = code
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "WS_ERR"), code, message))


class _Image(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("stride", ctypes.c_int)]


class _Params(ctypes.Structure):
    _fields_ = [("view", ctypes.c_int), ("cost", ctypes.c_int), ("block_size", ctypes.c_int),
                ("min_disparity", ctypes.c_int), ("max_disparity", ctypes.c_int),
                ("smooth_factor", ctypes.c_double), ("var_block", ctypes.c_int),
                ("thres", ctypes.c_double), ("subpixel", ctypes.c_int),
                ("linear_range", ctypes.c_int)]


class _OutliersPass(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("row_kernel", "row_passes", "row_per", "col_band", "row_window", "col_window")]


class _OutliersForms(ctypes.Structure):
    _fields_ = [("integer_pass", _OutliersPass), ("double_pass", _OutliersPass)]


class _LrParams(ctypes.Structure):
    _fields_ = [("max_diff", ctypes.c_float), ("fill", ctypes.c_int)]


LR_FILL_NONE, LR_FILL_BACKGROUND = 0, 1


def lr_params(max_diff=1.0, fill=False):
    """ws_lr_params: the largest |v - partner| that passes the left-right check; fill=True fills failed pixels from
    the nearest passed pixels of their row (WS_LR_FILL_BACKGROUND), else they become 0."""
    return _LrParams(max_diff, LR_FILL_BACKGROUND if fill else LR_FILL_NONE)


class _SpeckleParams(ctypes.Structure):
    _fields_ = [("new_val", ctypes.c_float), ("max_speckle_size", ctypes.c_int), ("max_diff", ctypes.c_float)]


def speckle_params(new_val=0.0, max_speckle_size=100, max_diff=1.0):
    """ws_speckle_params: regions of at most max_speckle_size pixels whose 4-neighbours differ by at most max_diff
    become new_val; pixels equal to new_val are blank (OpenCV's filterSpeckles)."""
    return _SpeckleParams(new_val, max_speckle_size, max_diff)


class _SgmParams(ctypes.Structure):
    _fields_ = [("paths", ctypes.c_int), ("p1", ctypes.c_int), ("p2", ctypes.c_int)]


def sgm_params(paths=8, p1=0, p2=0):
    """ws_sgm_params: 4 or 8 aggregation paths, the penalty p1 for a disparity change of 1 between path neighbours and
    p2 >= p1 for a larger one, in window-cost units (semi-global matching; rules in include/ws_stereo.h)."""
    return _SgmParams(paths, p1, p2)


def _image_struct(a):
    """A ws_image over an H x W x 3 uint8 array's rows (rows may be padded), without copying."""
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.strides[2] != 1 or a.strides[1] != 3:
        raise ValueError("expected an H x W x 3 uint8 (BGR) image with dense rows")
    return _Image(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0])


def validate_sgm(params, left, right, paths=8, p1=0, p2=0):
    """ws_validate_sgm on host images (H x W x 3 uint8): 0 or the WS_ERR_* status an SGM call would return."""
    lib = load_library()
    sp = sgm_params(paths, p1, p2)
    return int(lib.ws_validate_sgm(ctypes.byref(params), ctypes.byref(sp), ctypes.byref(_image_struct(left)),
                                   ctypes.byref(_image_struct(right))))


def sgm_scratch_bytes(params, left, right, paths=8, p1=0, p2=0):
    """ws_sgm_scratch_bytes: the device memory an SGM call on these images would hold (raises WsError if refused)."""
    lib = load_library()
    sp = sgm_params(paths, p1, p2)
    n = ctypes.c_ulonglong()
    rc = lib.ws_sgm_scratch_bytes(ctypes.byref(params), ctypes.byref(sp), ctypes.byref(_image_struct(left)),
                                  ctypes.byref(_image_struct(right)), ctypes.byref(n))
    if rc != 0:
        raise WsError(rc, lib.ws_last_error(None).decode())
    return int(n.value)


class _UniqueParams(ctypes.Structure):
    _fields_ = [("ratio", ctypes.c_int)]


def unique_params(ratio=0):
    """ws_unique_params: OpenCV's uniquenessRatio, 0 .. 100 (rules in include/ws_stereo.h)."""
    return _UniqueParams(ratio)


def _sgm_or_null(sgm):
    """sgm: None (the block route), a (paths, p1, p2) tuple or a ws_sgm_params -> (the struct kept alive, its pointer)."""
    if sgm is None:
        return None, None
    sp = sgm if isinstance(sgm, _SgmParams) else sgm_params(*sgm)
    return sp, ctypes.byref(sp)


def validate_unique(params, left, right, ratio=0, sgm=None):
    """ws_validate_unique on host images: 0 or the WS_ERR_* status a uniqueness call would return.  ratio None: a null
    ws_unique_params."""
    lib = load_library()
    sp, spp = _sgm_or_null(sgm)
    uq = None if ratio is None else unique_params(ratio)
    return int(lib.ws_validate_unique(ctypes.byref(params), spp, None if uq is None else ctypes.byref(uq),
                                      ctypes.byref(_image_struct(left)), ctypes.byref(_image_struct(right))))


def unique_scratch_bytes(params, left, right, sgm=None):
    """ws_unique_scratch_bytes: the device memory a uniqueness call on these images would hold (raises WsError if
    refused).  sgm None: the intervals and the cost plane only."""
    lib = load_library()
    sp, spp = _sgm_or_null(sgm)
    n = ctypes.c_ulonglong()
    rc = lib.ws_unique_scratch_bytes(ctypes.byref(params), spp, ctypes.byref(_image_struct(left)),
                                     ctypes.byref(_image_struct(right)), ctypes.byref(n))
    if rc != 0:
        raise WsError(rc, lib.ws_last_error(None).decode())
    return int(n.value)


def validate_pair(params, left, right, sgm=None, ratio=None, max_diff=None, fill=False):
    """ws_validate_pair on host images: 0 or the WS_ERR_* status a pair call would return.  ratio None: no uniqueness
    test; max_diff None: no left-right check."""
    lib = load_library()
    sp, spp = _sgm_or_null(sgm)
    uq = None if ratio is None else unique_params(ratio)
    lr = None if max_diff is None else lr_params(max_diff, fill)
    return int(lib.ws_validate_pair(ctypes.byref(params), spp, None if uq is None else ctypes.byref(uq),
                                    None if lr is None else ctypes.byref(lr), ctypes.byref(_image_struct(left)),
                                    ctypes.byref(_image_struct(right))))


class _Job(ctypes.Structure):
    _fields_ = [("params", _Params), ("left", _Image), ("right", _Image), ("out", ctypes.c_void_p),
                ("out_stride", ctypes.c_int), ("out_dtype", ctypes.c_int), ("status", ctypes.c_int)]


class _BatchItem(ctypes.Structure):
    _fields_ = [("job", ctypes.c_int), ("y0", ctypes.c_int), ("y1", ctypes.c_int), ("worker", ctypes.c_int)]


class _Calib(ctypes.Structure):
    _fields_ = [("cam0", ctypes.c_float * 9), ("cam1", ctypes.c_float * 9),
                ("doffs", ctypes.c_float), ("baseline", ctypes.c_float),
                ("width", ctypes.c_int), ("height", ctypes.c_int), ("ndisp", ctypes.c_int)]


class _PlanInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "marching", "x_per_thread", "d_per_thread", "x_runs", "d_chunks", "threads", "tiles",
        "strips", "strip_rows", "lds_bytes", "interior_x0", "interior_x1", "interior_y0",
        "interior_y1", "passes", "tile_cols", "kernel_kind")]


_lib = None


def _preload_hip_runtime():
    """Keep ONE HIP runtime in the process.  PyTorch-ROCm ships its own libamdhip64.so.7 (same
    SONAME as /opt/rocm's); if this library pulled in the system copy first, a later
    `import torch` would start a second HSA runtime and find no device.  So when PyTorch is
    installed but not imported yet, load the runtime it ships before libws_stereo.so."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def load_library(build_if_missing=False):
    """dlopen libws_stereo.so.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("WS_STEREO_LIB", _build.LIB)  # override: tuning variants only
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError("libws_stereo.so is missing: run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (the HIP extension is the only compute path)")
        _build.build()
    _preload_hip_runtime()
    lib = ctypes.CDLL(path)
    P, vp, ci = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int
    lib.ws_version.restype = ci
    lib.ws_params_default.argtypes = [P(_Params)]
    lib.ws_params_default.restype = None
    lib.ws_create.argtypes = [ci, P(vp)]
    lib.ws_destroy.argtypes = [vp]
    lib.ws_destroy.restype = None
    lib.ws_last_error.argtypes = [vp]
    lib.ws_last_error.restype = ctypes.c_char_p
    lib.ws_device_count.restype = ci
    lib.ws_validate.argtypes = [P(_Params), P(_Image), P(_Image)]
    lib.ws_plan.argtypes = [P(_Params), P(_Image), P(_Image), ci, P(_PlanInfo)]
    lib.ws_search_host.argtypes = [vp, P(_Params), P(_Image), P(_Image), vp, ci, ci]
    lib.ws_search_device.argtypes = [vp, P(_Params), P(_Image), P(_Image), vp, ci, vp]
    lib.ws_enqueue_host.argtypes = [vp, P(_Params), P(_Image), P(_Image), vp, ci, ci]
    lib.ws_wait.argtypes = [vp]
    cf = ctypes.c_float
    lib.ws_remove_disparity_outliers.argtypes = [vp, vp, ci, ci, ci, ci, cf, cf]
    lib.ws_convert_disparity_to_depth.argtypes = [vp, vp, ci, ci, ci, cf, cf, vp, ci]
    lib.ws_back_project.argtypes = [vp, vp, ci, ci, ci, P(cf), P(_Image), vp, vp]
    lib.ws_write_mesh_off.argtypes = [ctypes.c_char_p, vp, vp, ci, ci, cf]
    lib.ws_write_mesh_off_device.argtypes = [vp, vp, vp, ci, ci, cf, ctypes.c_char_p, vp]
    lib.ws_reconstruction_host.argtypes = [vp, vp, ci, ci, ci, P(cf), P(_Image), cf, ctypes.c_char_p]
    lib.ws_warp_nearest_host.argtypes = [vp, vp, ci, ci, ci, P(ctypes.c_double), vp, ci, ci, ci]
    lib.ws_warp_nearest_device.argtypes = [vp, vp, ci, ci, ci, P(ctypes.c_double), vp, ci, ci, ci, vp]
    lib.ws_timer_begin.argtypes = [vp, vp]
    lib.ws_timer_end.argtypes = [vp, vp, P(ctypes.c_float)]
    lib.ws_set_profiling.argtypes = [vp, ci]
    lib.ws_last_kernel_ms.argtypes = [vp, P(ctypes.c_float)]
    lib.ws_last_max_block.argtypes = [vp, ci, P(ci)]
    lib.ws_last_launch_info.argtypes = [vp, ctypes.c_char_p, ci, P(ci), P(ci), P(ci)]
    lib.ws_set_tuning.argtypes = [vp, ci, ci, ci]
    lib.ws_set_host_bands.argtypes = [vp, ci]
    lib.ws_last_host_paths.argtypes = [vp, P(ci)]
    lib.ws_last_wire_format.argtypes = [vp, P(ci)]
    lib.ws_last_outliers_path.argtypes = [vp, P(ci)]
    lib.ws_last_outliers_forms.argtypes = [vp, P(_OutliersForms)]
    lib.ws_device_status.argtypes = [vp, vp]
    lib.ws_pfm_read.argtypes = [ctypes.c_char_p, P(P(ctypes.c_float)), P(ci), P(ci)]
    lib.ws_pfm_write.argtypes = [ctypes.c_char_p, vp, ci, ci, ci]
    lib.ws_ppm_read.argtypes = [ctypes.c_char_p, P(P(ctypes.c_uint8)), P(ci), P(ci)]
    lib.ws_ppm_write.argtypes = [ctypes.c_char_p, vp, ci, ci, ci]
    lib.ws_free.argtypes = [vp]
    lib.ws_free.restype = None
    lib.ws_calib_read.argtypes = [ctypes.c_char_p, P(_Calib)]
    lib.ws_evaldisp.argtypes = [vp, vp, vp, ci, ci, ctypes.c_float, ctypes.c_float, ci,
                                P(ctypes.c_double)]
    D9 = P(ctypes.c_double)
    lib.ws_rectified_size.argtypes = [D9, ci, ci, P(ci), P(ci)]
    lib.ws_rectify_device.argtypes = [vp, P(_Image), D9, vp, ci, ci, ci, vp]
    lib.ws_search_unrectified_host.argtypes = [vp, P(_Params), P(_Image), P(_Image), D9, D9, vp, ci, ci, vp, ci, vp, ci]
    lib.ws_batch_create.argtypes = [P(ci), ci, P(vp)]
    lib.ws_batch_destroy.argtypes = [vp]
    lib.ws_batch_destroy.restype = None
    lib.ws_batch_last_error.argtypes = [vp]
    lib.ws_batch_last_error.restype = ctypes.c_char_p
    lib.ws_batch_workers.argtypes = [vp, P(ci), ci]
    lib.ws_batch_plan.argtypes = [P(_Job), ci, ci, ci, ci, P(_BatchItem), ci, P(ci), P(ci)]
    lib.ws_batch_search_host.argtypes = [vp, P(_Job), ci, ci, ci]
    lib.ws_lr_check_device.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci, ci, P(_LrParams), vp, ci, vp, ci, vp]
    lib.ws_search_lr_host.argtypes = [vp, P(_Params), P(_Image), P(_Image), P(_LrParams), vp, ci, vp, ci, ci]
    lib.ws_search_lr_device.argtypes = [vp, P(_Params), P(_Image), P(_Image), P(_LrParams), vp, ci, vp, ci, vp]
    lib.ws_last_lr_counts.argtypes = [vp, P(ctypes.c_ulonglong)]
    lib.ws_filter_speckles_device.argtypes = [vp, vp, ci, ci, ci, P(_SpeckleParams), vp]
    lib.ws_filter_speckles_host.argtypes = [vp, vp, ci, ci, ci, P(_SpeckleParams)]
    lib.ws_last_speckle_counts.argtypes = [vp, P(ctypes.c_ulonglong)]
    lib.ws_validate_sgm.argtypes = [P(_Params), P(_SgmParams), P(_Image), P(_Image)]
    lib.ws_sgm_scratch_bytes.argtypes = [P(_Params), P(_SgmParams), P(_Image), P(_Image), P(ctypes.c_ulonglong)]
    lib.ws_search_sgm_device.argtypes = [vp, P(_Params), P(_SgmParams), P(_Image), P(_Image), vp, ci, vp]
    lib.ws_search_sgm_host.argtypes = [vp, P(_Params), P(_SgmParams), P(_Image), P(_Image), vp, ci, ci]
    lib.ws_validate_unique.argtypes = [P(_Params), P(_SgmParams), P(_UniqueParams), P(_Image), P(_Image)]
    lib.ws_unique_scratch_bytes.argtypes = [P(_Params), P(_SgmParams), P(_Image), P(_Image), P(ctypes.c_ulonglong)]
    lib.ws_search_unique_device.argtypes = [vp, P(_Params), P(_SgmParams), P(_UniqueParams), P(_Image), P(_Image), vp, ci,
                                            vp, ci, vp]
    lib.ws_search_unique_host.argtypes = [vp, P(_Params), P(_SgmParams), P(_UniqueParams), P(_Image), P(_Image), vp, ci, ci,
                                          vp, ci]
    lib.ws_last_unique_counts.argtypes = [vp, P(ctypes.c_ulonglong)]
    lib.ws_validate_pair.argtypes = [P(_Params), P(_SgmParams), P(_UniqueParams), P(_LrParams), P(_Image), P(_Image)]
    lib.ws_search_pair_device.argtypes = [vp, P(_Params), P(_SgmParams), P(_UniqueParams), P(_LrParams), P(_Image), P(_Image),
                                          vp, ci, vp, ci, vp]
    lib.ws_search_pair_host.argtypes = [vp, P(_Params), P(_SgmParams), P(_UniqueParams), P(_LrParams), P(_Image), P(_Image),
                                        vp, ci, vp, ci, ci]
    lib.ws_census_transform_device.argtypes = [vp, P(_Image), ci, vp, ci, vp]
    lib.ws_census_transform_host.argtypes = [vp, P(_Image), ci, vp, ci]
    _lib = lib
    return lib


def device_count():
    """ws_device_count: the HIP devices this process sees (0 without one; never raises)."""
    return int(load_library().ws_device_count())


def make_params(view, block_size=7, min_disparity=0, max_disparity=64, smooth_factor=1.0,
                cost="ssd", var_block=False, thres=19.0, subpixel=False, linear_range=200):
    p = _Params()
    load_library().ws_params_default(ctypes.byref(p))
    p.view, p.cost = view, _COST[cost]
    p.block_size, p.min_disparity, p.max_disparity = block_size, min_disparity, max_disparity
    p.smooth_factor, p.var_block, p.thres = smooth_factor, int(var_block), thres
    p.subpixel, p.linear_range = int(subpixel), linear_range
    return p


def _host_image(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected an H x W x 3 uint8 (BGR) image")
    return a, _Image(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0])


class WindowSearch:
    """One ws_context: a HIP device, its stream and scratch memory."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.ws_create(device, ctypes.byref(h))
        if rc != 0:
            raise WsError(rc, self._lib.ws_last_error(None).decode())
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ws_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise WsError(rc, self._lib.ws_last_error(self._h).decode())

    # -- host buffers (numpy in, numpy out) ------------------------------------------------
    def search(self, params, left, right, dtype=np.float64, out=None):
        """ws_search_host.  `out`: a C-contiguous float32 / float64 array of the map's shape to write into
        (a caller that keeps its output buffer); by default a fresh array per call, as the reference returns."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        shape = La.shape[:2] if params.view == VIEW_LEFT else Ra.shape[:2]
        if out is None:
            out = np.empty(shape, dtype=dtype)
        elif out.shape != shape or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous array of shape %s" % (shape,))
        code = OUT_F64 if out.dtype == np.float64 else OUT_F32
        if out.dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        self._check(self._lib.ws_search_host(self._h, ctypes.byref(params), ctypes.byref(Li),
                                             ctypes.byref(Ri), out.ctypes.data, shape[1], code))
        return out

    def search_many(self, params, pairs, dtype=np.float32):
        """Batched host path (ws_enqueue_host / ws_wait) over independent pairs.  Whatever happens, nothing is
        dropped before ws_wait has returned: the library copies from / into these buffers until then."""
        keep, outs = [], []
        try:
            for left, right in pairs:
                La, Li = _host_image(left)
                Ra, Ri = _host_image(right)
                shape = La.shape[:2] if params.view == VIEW_LEFT else Ra.shape[:2]
                out = np.empty(shape, dtype=dtype)
                code = OUT_F64 if out.dtype == np.float64 else OUT_F32
                keep.append((La, Ra, Li, Ri))
                outs.append(out)
                self._check(self._lib.ws_enqueue_host(self._h, ctypes.byref(params), ctypes.byref(Li),
                                                      ctypes.byref(Ri), out.ctypes.data, shape[1], code))
        except BaseException:
            self._lib.ws_wait(self._h)  # the pairs already enqueued still copy from / into keep and outs
            raise
        self._check(self._lib.ws_wait(self._h))
        del keep
        return outs

    # -- device buffers (torch tensors already in HBM) -------------------------------------
    def search_device(self, params, left_t, right_t, out_t, stream=None, check=False):
        """left_t/right_t: uint8 CUDA tensors H x W x 3 (contiguous rows); out_t: float32 H x W.
        Only enqueues.  The one thing a kernel can report after the fact -- the left view's smoothFactor raster pass
        giving up on the band above it, the map is then invalid -- surfaces in the next call that synchronises:
        device_status(stream), or this call with check=True (waits for the stream and raises).  A caller that
        synchronises with torch alone must call device_status() before trusting a left-view smoothFactor != 1 map."""
        Li = _Image(left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0))
        Ri = _Image(right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0))
        self._check(self._lib.ws_search_device(self._h, ctypes.byref(params), ctypes.byref(Li),
                                               ctypes.byref(Ri), out_t.data_ptr(), out_t.stride(0),
                                               ctypes.c_void_p(stream or 0)))
        if check:
            self.device_status(stream)

    # -- left-right consistency check (extension; rules in include/ws_stereo.h) -------------------
    def search_lr(self, params, left, right, max_diff=1.0, fill=False, dtype=np.float64):
        """ws_search_lr_host: both block-search views of the pair (params.view is ignored), then the left-right check.
        Returns (left_map, right_map); failed pixels are 0, or filled from their row's passed pixels with fill=True."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        outl = np.empty(La.shape[:2], dtype=dtype)
        outr = np.empty(Ra.shape[:2], dtype=dtype)
        lr = lr_params(max_diff, fill)
        self._check(self._lib.ws_search_lr_host(self._h, ctypes.byref(params), ctypes.byref(Li), ctypes.byref(Ri),
                                                ctypes.byref(lr), outl.ctypes.data, outl.shape[1], outr.ctypes.data,
                                                outr.shape[1], OUT_F64 if dtype == np.float64 else OUT_F32))
        return outl, outr

    def search_lr_device(self, params, left_t, right_t, out_left_t, out_right_t, max_diff=1.0, fill=False, stream=None,
                         check=False):
        """ws_search_lr_device on uint8 CUDA images and float32 CUDA maps (as search_device).  Only enqueues."""
        Li = _Image(left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0))
        Ri = _Image(right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0))
        lr = lr_params(max_diff, fill)
        self._check(self._lib.ws_search_lr_device(self._h, ctypes.byref(params), ctypes.byref(Li), ctypes.byref(Ri),
                                                  ctypes.byref(lr), out_left_t.data_ptr(), out_left_t.stride(0),
                                                  out_right_t.data_ptr(), out_right_t.stride(0), ctypes.c_void_p(stream or 0)))
        if check:
            self.device_status(stream)

    def lr_check_device(self, left_t, right_t, out_left_t, out_right_t, max_diff=1.0, fill=False, stream=None):
        """ws_lr_check_device on float32 CUDA maps (H x W, rows may be padded).  Only enqueues on `stream`."""
        for t in (left_t, right_t, out_left_t, out_right_t):
            if t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 4 or not t.is_floating_point():
                raise ValueError("expected float32 H x W tensors with dense rows")
        lr = lr_params(max_diff, fill)
        self._check(self._lib.ws_lr_check_device(
            self._h, left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0),
            right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0), ctypes.byref(lr),
            out_left_t.data_ptr(), out_left_t.stride(0), out_right_t.data_ptr(), out_right_t.stride(0),
            ctypes.c_void_p(stream or 0)))

    def last_lr_counts(self):
        """ws_last_lr_counts: (failed pixels of the left map, of the right map) in the last check of this context."""
        c = (ctypes.c_ulonglong * 2)()
        self._check(self._lib.ws_last_lr_counts(self._h, c))
        return int(c[0]), int(c[1])

    # -- semi-global matching (extension; rules in include/ws_stereo.h) --------------------------
    def search_sgm(self, params, left, right, paths=8, p1=0, p2=0, dtype=np.float64, out=None):
        """ws_search_sgm_host: the view's map with the window costs aggregated along `paths` image paths (penalties
        p1, p2).  `out` as for search()."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        shape = La.shape[:2] if params.view == VIEW_LEFT else Ra.shape[:2]
        if out is None:
            out = np.empty(shape, dtype=dtype)
        elif out.shape != shape or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous array of shape %s" % (shape,))
        if out.dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        sp = sgm_params(paths, p1, p2)
        self._check(self._lib.ws_search_sgm_host(self._h, ctypes.byref(params), ctypes.byref(sp), ctypes.byref(Li),
                                                 ctypes.byref(Ri), out.ctypes.data, shape[1],
                                                 OUT_F64 if out.dtype == np.float64 else OUT_F32))
        return out

    def search_sgm_device(self, params, left_t, right_t, out_t, paths=8, p1=0, p2=0, stream=None):
        """ws_search_sgm_device on uint8 CUDA images and a float32 CUDA map (as search_device).  Only enqueues."""
        Li = _Image(left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0))
        Ri = _Image(right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0))
        sp = sgm_params(paths, p1, p2)
        self._check(self._lib.ws_search_sgm_device(self._h, ctypes.byref(params), ctypes.byref(sp), ctypes.byref(Li),
                                                   ctypes.byref(Ri), out_t.data_ptr(), out_t.stride(0),
                                                   ctypes.c_void_p(stream or 0)))

    # -- uniqueness ratio and confidence (extension; rules in include/ws_stereo.h) ----------------
    def search_unique(self, params, left, right, ratio, sgm=None, dtype=np.float64, out=None, conf=False):
        """ws_search_unique_host: the view's map with the nodes that fail the uniqueness test at `ratio` set to 0.  sgm:
        None for the block search's costs, or (paths, p1, p2) for semi-global matching.  `out` as for search().  conf:
        True returns (map, confidence) with a fresh float32 plane; a C-contiguous float32 array of the map's shape is
        written into and returned the same way."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        shape = La.shape[:2] if params.view == VIEW_LEFT else Ra.shape[:2]
        if out is None:
            out = np.empty(shape, dtype=dtype)
        elif out.shape != shape or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous array of shape %s" % (shape,))
        if out.dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        if conf is True:
            conf = np.empty(shape, dtype=np.float32)
        elif conf is False or conf is None:
            conf = None
        elif conf.shape != shape or conf.dtype != np.float32 or not conf.flags["C_CONTIGUOUS"]:
            raise ValueError("conf must be a C-contiguous float32 array of shape %s" % (shape,))
        sp, spp = _sgm_or_null(sgm)
        uq = unique_params(ratio)
        self._check(self._lib.ws_search_unique_host(self._h, ctypes.byref(params), spp, ctypes.byref(uq), ctypes.byref(Li),
                                                    ctypes.byref(Ri), out.ctypes.data, shape[1],
                                                    OUT_F64 if out.dtype == np.float64 else OUT_F32,
                                                    None if conf is None else conf.ctypes.data, shape[1]))
        return out if conf is None else (out, conf)

    def search_unique_device(self, params, left_t, right_t, out_t, ratio, sgm=None, conf_t=None, stream=None):
        """ws_search_unique_device on uint8 CUDA images, a float32 CUDA map and, if given, a float32 CUDA confidence
        plane (rows may be padded).  Only enqueues."""
        Li = _Image(left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0))
        Ri = _Image(right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0))
        sp, spp = _sgm_or_null(sgm)
        uq = unique_params(ratio)
        self._check(self._lib.ws_search_unique_device(
            self._h, ctypes.byref(params), spp, ctypes.byref(uq), ctypes.byref(Li), ctypes.byref(Ri), out_t.data_ptr(),
            out_t.stride(0), None if conf_t is None else conf_t.data_ptr(), 0 if conf_t is None else conf_t.stride(0),
            ctypes.c_void_p(stream or 0)))

    def last_unique_counts(self):
        """ws_last_unique_counts: (failed nodes, nodes) of the last uniqueness call of this context."""
        c = (ctypes.c_ulonglong * 2)()
        self._check(self._lib.ws_last_unique_counts(self._h, c))
        return int(c[0]), int(c[1])

    # -- both views from one volume (extension; rules in include/ws_stereo.h) ---------------------
    def search_pair(self, params, left, right, sgm=None, ratio=None, max_diff=None, fill=False, dtype=np.float64):
        """ws_search_pair_host: the base view's map (params.view; as search_sgm / search_unique / search compute it)
        and the other view's map derived from the same sums, as (left_map, right_map).  sgm: None for the block
        search's costs or (paths, p1, p2); ratio: None or the uniqueness ratio of the base winner; max_diff: None for
        the raw maps, else the two are left-right checked (fill as for search_lr)."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        outl = np.empty(La.shape[:2], dtype=dtype)
        outr = np.empty(Ra.shape[:2], dtype=dtype)
        sp, spp = _sgm_or_null(sgm)
        uq = None if ratio is None else unique_params(ratio)
        lr = None if max_diff is None else lr_params(max_diff, fill)
        self._check(self._lib.ws_search_pair_host(
            self._h, ctypes.byref(params), spp, None if uq is None else ctypes.byref(uq),
            None if lr is None else ctypes.byref(lr), ctypes.byref(Li), ctypes.byref(Ri), outl.ctypes.data, outl.shape[1],
            outr.ctypes.data, outr.shape[1], OUT_F64 if dtype == np.float64 else OUT_F32))
        return outl, outr

    def search_pair_device(self, params, left_t, right_t, out_left_t, out_right_t, sgm=None, ratio=None, max_diff=None,
                           fill=False, stream=None):
        """ws_search_pair_device on uint8 CUDA images and two float32 CUDA maps (rows may be padded).  Only enqueues."""
        Li = _Image(left_t.data_ptr(), left_t.shape[1], left_t.shape[0], left_t.stride(0))
        Ri = _Image(right_t.data_ptr(), right_t.shape[1], right_t.shape[0], right_t.stride(0))
        sp, spp = _sgm_or_null(sgm)
        uq = None if ratio is None else unique_params(ratio)
        lr = None if max_diff is None else lr_params(max_diff, fill)
        self._check(self._lib.ws_search_pair_device(
            self._h, ctypes.byref(params), spp, None if uq is None else ctypes.byref(uq),
            None if lr is None else ctypes.byref(lr), ctypes.byref(Li), ctypes.byref(Ri), out_left_t.data_ptr(),
            out_left_t.stride(0), out_right_t.data_ptr(), out_right_t.stride(0), ctypes.c_void_p(stream or 0)))

    # -- census transform (extension; rules in include/ws_stereo.h) -------------------------------
    def census_transform(self, img, cost):
        """ws_census_transform_host: the census descriptors of a BGR image (H x W x 3 uint8) as an H x W uint64 array;
        cost is COST_CENSUS_5X5 / COST_CENSUS_9X7 or "census5x5" / "census9x7"."""
        a, hdr = _host_image(img)
        out = np.empty(a.shape[:2], dtype=np.uint64)
        self._check(self._lib.ws_census_transform_host(self._h, ctypes.byref(hdr), _COST[cost], out.ctypes.data, out.shape[1]))
        return out

    def census_transform_device(self, img_t, cost, out_t, stream=None):
        """ws_census_transform_device on a uint8 CUDA image H x W x 3 into a 64-bit integer CUDA tensor H x W (rows may
        be padded).  Only enqueues on `stream` (as search_device)."""
        if out_t.dim() != 2 or out_t.stride(1) != 1 or out_t.element_size() != 8 or out_t.is_floating_point():
            raise ValueError("expected a 64-bit integer H x W tensor with dense rows")
        Ii = _Image(img_t.data_ptr(), img_t.shape[1], img_t.shape[0], img_t.stride(0))
        self._check(self._lib.ws_census_transform_device(self._h, ctypes.byref(Ii), _COST[cost], out_t.data_ptr(),
                                                         out_t.stride(0), ctypes.c_void_p(stream or 0)))

    # -- speckle filter (extension; rules in include/ws_stereo.h) ---------------------------------
    def filter_speckles(self, disparity, new_val=0.0, max_speckle_size=100, max_diff=1.0):
        """ws_filter_speckles_host on a float32 copy of `disparity` (OpenCV's filterSpeckles); returns the copy."""
        m = np.array(disparity, dtype=np.float32, order="C")
        if m.ndim != 2:
            raise ValueError("expected an H x W map")
        sp = speckle_params(new_val, max_speckle_size, max_diff)
        self._check(self._lib.ws_filter_speckles_host(self._h, m.ctypes.data, m.shape[1], m.shape[0], m.shape[1],
                                                      ctypes.byref(sp)))
        return m

    def filter_speckles_device(self, t, new_val=0.0, max_speckle_size=100, max_diff=1.0, stream=None):
        """ws_filter_speckles_device in place on a float32 CUDA map (H x W, rows may be padded).  Only enqueues."""
        if t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 4 or not t.is_floating_point():
            raise ValueError("expected a float32 H x W tensor with dense rows")
        sp = speckle_params(new_val, max_speckle_size, max_diff)
        self._check(self._lib.ws_filter_speckles_device(self._h, t.data_ptr(), t.shape[1], t.shape[0], t.stride(0),
                                                        ctypes.byref(sp), ctypes.c_void_p(stream or 0)))

    def last_speckle_counts(self):
        """ws_last_speckle_counts: (pixels set to new_val, regions removed) by the last filter of this context."""
        c = (ctypes.c_ulonglong * 2)()
        self._check(self._lib.ws_last_speckle_counts(self._h, c))
        return int(c[0]), int(c[1])

    def warp_nearest(self, src, matrix, dst_shape):
        """cv::warpPerspective(src, dst, matrix, dst_size, INTER_NEAREST) on a float64 map."""
        a = np.ascontiguousarray(src, dtype=np.float64)
        m = (ctypes.c_double * 9)(*np.asarray(matrix, dtype=np.float64).reshape(9))
        out = np.empty(dst_shape, dtype=np.float64)
        self._check(self._lib.ws_warp_nearest_host(self._h, a.ctypes.data, a.shape[1], a.shape[0], a.shape[1],
                                                   m, out.ctypes.data, out.shape[1], out.shape[0], out.shape[1]))
        return out

    def warp_nearest_device(self, src_t, matrix, dst_t, stream=None):
        """ws_warp_nearest_device: the same warp between float32 CUDA maps (H x W, rows may be padded).  Only enqueues on
        `stream`, a hipStream_t handle (None or 0: the context's own NON-BLOCKING stream, see rectify_device)."""
        for t in (src_t, dst_t):
            if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 4 or not t.is_floating_point():
                raise ValueError("expected a float32 H x W CUDA tensor with dense rows")
        self._check(self._lib.ws_warp_nearest_device(self._h, src_t.data_ptr(), src_t.shape[1], src_t.shape[0],
                                                     src_t.stride(0), _mat9(matrix), dst_t.data_ptr(), dst_t.shape[1],
                                                     dst_t.shape[0], dst_t.stride(0), ctypes.c_void_p(stream or 0)))

    # -- rectification (rectification.cpp:432-505, :66-88) ----------------------------------
    def rectify_device(self, src_t, H, dst_t, stream=None):
        """ws_rectify_device: cv::warpPerspective(src, dst, H, dst.size()) -- INTER_LINEAR, BORDER_CONSTANT 0 -- on
        uint8 CUDA tensors H x W x 3 (rows may be padded: row stride >= 3 * width, pixels and channels dense).
        Only enqueues on `stream`, a hipStream_t handle.  The default (None or 0) is the context's own stream, which is
        NON-BLOCKING: it is not ordered against torch's null stream.  Pass the stream the tensors were written on
        (torch.cuda.current_stream().cuda_stream when that is not the null stream) or synchronise before and after."""
        for t in (src_t, dst_t):
            if t.dtype != _uint8_dtype(t) or not t.is_cuda:
                raise ValueError("expected a uint8 CUDA tensor, got %s on %s" % (t.dtype, t.device))
            if t.dim() != 3 or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3:
                raise ValueError("expected an H x W x 3 uint8 tensor with dense pixels")
        Si = _Image(src_t.data_ptr(), src_t.shape[1], src_t.shape[0], src_t.stride(0))
        self._check(self._lib.ws_rectify_device(self._h, ctypes.byref(Si), _mat9(H), dst_t.data_ptr(), dst_t.shape[1],
                                                dst_t.shape[0], dst_t.stride(0), ctypes.c_void_p(stream or 0)))

    def search_unrectified(self, params, left, right, H, Hp, dtype=np.float64, rectified=False):
        """ws_search_unrectified_host: rectify both images on the device (left with H = H_, right with Hp = Hp_), search,
        warp the map back with H_.inv() to the original frame.  Returns the map, or (map, rect_left, rect_right) with
        rectified=True."""
        La, Li = _host_image(left)
        Ra, Ri = _host_image(right)
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be float32 or float64")
        shape = La.shape[:2] if params.view == VIEW_LEFT else Ra.shape[:2]
        out = np.empty(shape, dtype=dtype)
        rl = rr = None
        if rectified:
            rl = np.empty(rectified_size(H, La.shape) + (3,), dtype=np.uint8)
            rr = np.empty(rectified_size(Hp, Ra.shape) + (3,), dtype=np.uint8)
        self._check(self._lib.ws_search_unrectified_host(
            self._h, ctypes.byref(params), ctypes.byref(Li), ctypes.byref(Ri), _mat9(H), _mat9(Hp), out.ctypes.data,
            shape[1], OUT_F64 if out.dtype == np.float64 else OUT_F32,
            rl.ctypes.data if rectified else None, rl.strides[0] if rectified else 0,
            rr.ctypes.data if rectified else None, rr.strides[0] if rectified else 0))
        return (out, rl, rr) if rectified else out

    # -- consumers (Reconstruction side) ---------------------------------------------------
    def remove_disparity_outliers(self, disparity, kernel_size, thr_front, thr_back):
        m = np.array(disparity, dtype=np.float32, order="C")
        self._check(self._lib.ws_remove_disparity_outliers(self._h, m.ctypes.data, m.shape[1], m.shape[0], m.shape[1],
                                                           kernel_size, thr_front, thr_back))
        return m

    def convert_disparity_to_depth(self, disparity, focal_length, baseline):
        d = np.ascontiguousarray(disparity, dtype=np.float32)
        out = np.empty_like(d)
        self._check(self._lib.ws_convert_disparity_to_depth(self._h, d.ctypes.data, d.shape[1], d.shape[0], d.shape[1],
                                                            focal_length, baseline, out.ctypes.data, out.shape[1]))
        return out

    def back_project(self, depth, intrinsics, bgr):
        z = np.ascontiguousarray(depth, dtype=np.float32)
        img, hdr = _host_image(bgr)
        k = (ctypes.c_float * 9)(*np.asarray(intrinsics, dtype=np.float32).reshape(9))
        pos = np.empty(z.shape + (4,), dtype=np.float32)
        col = np.empty(z.shape + (4,), dtype=np.uint8)
        self._check(self._lib.ws_back_project(self._h, z.ctypes.data, z.shape[1], z.shape[0], z.shape[1], k,
                                              ctypes.byref(hdr), pos.ctypes.data, col.ctypes.data))
        return pos, col

    def reconstruction(self, depth, intrinsics, bgr, edge_threshold, path):
        """ws_reconstruction_host: reconstruction(bgrImage, depthValues, intrinsics, thrMesh) (reconstruction.cpp:152-208)
        -- back-projection and the COFF mesh text on the device, the file written at `path`.  The same bytes as
        back_project() followed by write_mesh_off()."""
        z = np.ascontiguousarray(depth, dtype=np.float32)
        img, hdr = _host_image(bgr)
        k = (ctypes.c_float * 9)(*np.asarray(intrinsics, dtype=np.float32).reshape(9))
        self._check(self._lib.ws_reconstruction_host(self._h, z.ctypes.data, z.shape[1], z.shape[0], z.shape[1], k,
                                                     ctypes.byref(hdr), edge_threshold, os.fsencode(path)))

    def write_mesh_off_device(self, positions_t, colors_t, edge_threshold, path, stream=None):
        """ws_write_mesh_off_device: write_mesh_off() of vertex buffers on the device -- positions_t a float32 CUDA tensor
        H x W x 4, colors_t a uint8 CUDA tensor H x W x 4, both contiguous.  Orders after `stream` (a hipStream_t handle;
        None = the context's own, NON-BLOCKING stream: pass torch.cuda.current_stream().cuda_stream or synchronise
        first) and returns once the file is written."""
        for t, dt, what in ((positions_t, "float32", "positions"), (colors_t, "uint8", "colors")):
            if not t.is_cuda or str(t.dtype) != "torch." + dt:
                raise ValueError("%s: expected a %s CUDA tensor, got %s on %s" % (what, dt, t.dtype, t.device))
            if t.dim() != 3 or t.shape[2] != 4 or not t.is_contiguous():
                raise ValueError("%s: expected a contiguous H x W x 4 tensor" % what)
        if tuple(positions_t.shape) != tuple(colors_t.shape):
            raise ValueError("positions and colors differ in shape")
        h, w = positions_t.shape[:2]
        self._check(self._lib.ws_write_mesh_off_device(self._h, positions_t.data_ptr(), colors_t.data_ptr(), w, h,
                                                       edge_threshold, os.fsencode(path), ctypes.c_void_p(stream or 0)))

    def timer_begin(self, stream=None):
        self._check(self._lib.ws_timer_begin(self._h, ctypes.c_void_p(stream or 0)))

    def timer_end(self, stream=None):
        ms = ctypes.c_float()
        self._check(self._lib.ws_timer_end(self._h, ctypes.c_void_p(stream or 0), ctypes.byref(ms)))
        return ms.value

    def set_profiling(self, enable):
        self._check(self._lib.ws_set_profiling(self._h, int(bool(enable))))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self._check(self._lib.ws_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def last_launch(self):
        name = ctypes.create_string_buffer(128)
        t, w, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.ws_last_launch_info(self._h, name, 128, ctypes.byref(t),
                                                  ctypes.byref(w), ctypes.byref(l)))
        return {"kernel": name.value.decode(), "threads": t.value, "workgroups": w.value,
                "lds_bytes": l.value}

    def last_max_block(self, block_size):
        v = ctypes.c_int()
        self._check(self._lib.ws_last_max_block(self._h, block_size, ctypes.byref(v)))
        return v.value

    def device_status(self, stream=None):
        """ws_device_status: wait for the stream and raise if a kernel flagged trouble since the last check."""
        self._check(self._lib.ws_device_status(self._h, ctypes.c_void_p(stream or 0)))

    def last_host_paths(self):
        """How the last host call's (left, right, out) bytes crossed: 'gathered', 'caller-pinned', 'staged'
        ('registered': rounds 2-3 only -- the library registers no caller memory any more)."""
        how = (ctypes.c_int * 3)()
        self._check(self._lib.ws_last_host_paths(self._h, how))
        return tuple(("gathered", "registered", "caller-pinned", "staged")[v] for v in how)

    def last_wire_format(self):
        """The format the last ws_search_host map crossed PCIe in: 'int16' (widened on the host) or 'float32'."""
        v = ctypes.c_int(0)
        self._check(self._lib.ws_last_wire_format(self._h, ctypes.byref(v)))
        return ("same", "int16", "float32")[v.value]

    def last_outliers_path(self):
        """Which box filter the last remove_disparity_outliers ran: 'double', 'integer', 'integer-then-double'."""
        v = ctypes.c_int(0)
        self._check(self._lib.ws_last_outliers_path(self._h, ctypes.byref(v)))
        return ("double", "integer", "integer-then-double")[v.value]

    def last_outliers_forms(self):
        """ws_last_outliers_forms: which kernel forms the last remove_disparity_outliers launched, as
        {'integer': pass or None, 'double': pass or None}; a pass is {'rows': 'u32' / 'lds-prefix' / 'direct',
        'row_passes', 'row_per', 'cols': the band width or 'direct', 'row_window', 'col_window': 'short' / 'periodic'}."""
        f = _OutliersForms()
        self._check(self._lib.ws_last_outliers_forms(self._h, ctypes.byref(f)))

        def one(p):
            if not p.row_kernel:
                return None
            return {"rows": (None, "u32", "lds-prefix", "direct")[p.row_kernel], "row_passes": p.row_passes,
                    "row_per": p.row_per, "cols": p.col_band or "direct",
                    "row_window": (None, "short", "periodic")[p.row_window],
                    "col_window": (None, "short", "periodic")[p.col_window]}
        return {"integer": one(f.integer_pass), "double": one(f.double_pass)}

    def set_host_bands(self, bands=-1):
        self._check(self._lib.ws_set_host_bands(self._h, bands))

    def set_tuning(self, x_runs_per_tile=0, strip_rows=0, threads=0):
        self._check(self._lib.ws_set_tuning(self._h, x_runs_per_tile, strip_rows, threads))


def _param_list(params_or_list, n):
    if isinstance(params_or_list, (list, tuple)):
        if len(params_or_list) != n:
            raise ValueError("%d parameter sets for %d pairs" % (len(params_or_list), n))
        return list(params_or_list)
    return [params_or_list] * n


def batch_plan(params_or_list, shapes, n_workers, bands=True, min_rows=256):
    """ws_batch_plan: the items a BatchSearch of n_workers workers would run on pairs of these shapes, without a device.
    shapes: per pair ((left rows, cols), (right rows, cols)), or one (rows, cols) for both images.  Returns
    (items, banded): items = [(job, y0, y1, worker)] grouped by worker -- map rows [y0, y1) of pair `job` --, banded =
    whether the batch was cut into row bands (sharding.band_items) rather than dealt as whole pairs (sharding.lpt_assign)."""
    shapes = [s if isinstance(s[0], (tuple, list)) else (s, s) for s in shapes]
    plist = _param_list(params_or_list, len(shapes))
    jobs = (_Job * max(1, len(shapes)))()
    for k, ((ls, rs), p) in enumerate(zip(shapes, plist)):
        jobs[k].params, jobs[k].left, jobs[k].right = p, _shape_image(ls), _shape_image(rs)
    cap = len(shapes) + max(1, n_workers)
    items = (_BatchItem * cap)()
    n, banded = ctypes.c_int(), ctypes.c_int()
    lib = load_library()
    rc = lib.ws_batch_plan(jobs, len(shapes), n_workers, int(bool(bands)), min_rows, items, cap, ctypes.byref(n),
                           ctypes.byref(banded))
    if rc != 0:
        raise WsError(rc, lib.ws_batch_last_error(None).decode())
    return [(it.job, it.y0, it.y1, it.worker) for it in items[:n.value]], bool(banded.value)


class BatchSearch:
    """Many independent pairs over several devices (ws_batch_*): one worker -- a context and a host thread -- per entry
    of `devices` (a device may repeat; None = one per device of the node).  Pairs are dealt as whole pairs (LPT) or as
    row bands (sharding.band_items); every map equals WindowSearch.search of that pair."""

    def __init__(self, devices=None):
        self._lib = load_library()
        h = ctypes.c_void_p()
        if devices is None:
            rc = self._lib.ws_batch_create(None, 0, ctypes.byref(h))
        else:
            devices = [int(d) for d in devices]
            arr = (ctypes.c_int * max(1, len(devices)))(*devices)
            rc = self._lib.ws_batch_create(arr, len(devices), ctypes.byref(h))
        if rc != 0:
            raise WsError(rc, self._lib.ws_batch_last_error(None).decode())
        self._h = h
        n = self._lib.ws_batch_workers(self._h, None, 0)
        arr = (ctypes.c_int * max(1, n))()
        self._lib.ws_batch_workers(self._h, arr, n)
        self.workers = list(arr[:n])

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ws_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def plan(self, params_or_list, pairs, bands=True, min_rows=256):
        """What search() would run on these pairs (image arrays or shapes): ([(job, y0, y1, worker)], banded)."""
        shapes = [p if isinstance(p[0], (tuple, list)) else (p[0].shape[:2], p[1].shape[:2]) for p in pairs]
        return batch_plan(params_or_list, shapes, len(self.workers), bands, min_rows)

    def search(self, params_or_list, pairs, dtype=np.float32, bands=True, min_rows=256, outs=None):
        """ws_batch_search_host: the maps of all pairs (one params for all, or one per pair).  `outs`: C-contiguous
        float32 / float64 arrays of the maps' shapes to write into instead of fresh ones.  Raises WsError with the first
        failed job's status; every array stays alive until the call has returned."""
        plist = _param_list(params_or_list, len(pairs))
        jobs = (_Job * max(1, len(pairs)))()
        keep, maps = [], []
        for k, ((left, right), p) in enumerate(zip(pairs, plist)):
            La, Li = _host_image(left)
            Ra, Ri = _host_image(right)
            shape = La.shape[:2] if p.view == VIEW_LEFT else Ra.shape[:2]
            out = np.empty(shape, dtype=dtype) if outs is None else outs[k]
            if out.shape != shape or not out.flags["C_CONTIGUOUS"] or out.dtype not in (np.float32, np.float64):
                raise ValueError("out %d must be a C-contiguous float32 / float64 array of shape %s" % (k, shape))
            keep.append((La, Ra))
            maps.append(out)
            jobs[k].params, jobs[k].left, jobs[k].right = p, Li, Ri
            jobs[k].out, jobs[k].out_stride = out.ctypes.data, shape[1]
            jobs[k].out_dtype = OUT_F64 if out.dtype == np.float64 else OUT_F32
        rc = self._lib.ws_batch_search_host(self._h, jobs, len(pairs), int(bool(bands)), min_rows)
        self.statuses = [jobs[k].status for k in range(len(pairs))]
        del keep
        if rc != 0:
            raise WsError(rc, self._lib.ws_batch_last_error(self._h).decode())
        return maps


def _shape_image(shape):
    """An image header with a non-null dummy pointer: enough for the device-free checks."""
    h, w = shape[:2]
    return _Image(1, w, h, 3 * w)


def validate(params, left_shape, right_shape):
    """Status code the search would return for these arguments (no device needed)."""
    Li, Ri = _shape_image(left_shape), _shape_image(right_shape)
    return load_library().ws_validate(ctypes.byref(params), ctypes.byref(Li), ctypes.byref(Ri))


def plan(params, left_shape, right_shape, num_cus=256):
    """Tiling the library would use (host logic only, no device needed)."""
    Li, Ri = _shape_image(left_shape), _shape_image(right_shape)
    info = _PlanInfo()
    rc = load_library().ws_plan(ctypes.byref(params), ctypes.byref(Li), ctypes.byref(Ri), num_cus,
                                ctypes.byref(info))
    if rc != 0:
        raise WsError(rc, load_library().ws_last_error(None).decode())
    return {n: getattr(info, n) for n, _ in _PlanInfo._fields_}


def _uint8_dtype(t):
    import torch  # (only reached with a torch tensor in hand)
    return torch.uint8


def _mat9(m):
    a = np.asarray(m, dtype=np.float64).reshape(9)
    return (ctypes.c_double * 9)(*a)


def rectified_size(H, shape):
    """ws_rectified_size: (rows, cols) of the image of shape (rows, cols[, 3]) rectified with H
    (rectification.cpp:436-483; not translated by min_x / min_y, as in the reference).  No device needed."""
    lib = load_library()
    w, h = ctypes.c_int(), ctypes.c_int()
    rc = lib.ws_rectified_size(_mat9(H), int(shape[1]), int(shape[0]), ctypes.byref(w), ctypes.byref(h))
    if rc != 0:
        raise WsError(rc, lib.ws_last_error(None).decode())
    return (h.value, w.value)


_default_ctx = None


def _ctx(ctx):
    global _default_ctx
    if ctx is not None:
        return ctx
    if _default_ctx is None:
        _default_ctx = WindowSearch(0)
    return _default_ctx


class BlockSearch:
    """Mirror of the reference's BlockSearch (BlockSearch.h:9-46); `cost`, `subpixel` and
    `context` are the build's additions."""

    def __init__(self, leftImage, rightImage, blockSize, minDisparity, maxDisparity,
                 cost="ssd", subpixel=False, context=None):
        self.leftImage_, self.rightImage_ = leftImage, rightImage
        self.blockSize_, self.minDisparity_, self.maxDisparity_ = blockSize, minDisparity, maxDisparity
        self.cost, self.subpixel, self._context = cost, subpixel, context

    def computeDisparityMapLeft(self, smoothFactor):
        p = make_params(VIEW_LEFT, self.blockSize_, self.minDisparity_, self.maxDisparity_,
                        smoothFactor, self.cost, subpixel=self.subpixel)
        return _ctx(self._context).search(p, self.leftImage_, self.rightImage_)

    def computeDisparityMapRight(self, smoothFactor, varBlock=False, thres=19.0):
        p = make_params(VIEW_RIGHT, self.blockSize_, self.minDisparity_, self.maxDisparity_,
                        smoothFactor, self.cost, varBlock, thres, self.subpixel)
        return _ctx(self._context).search(p, self.leftImage_, self.rightImage_)

    def computeDisparityMapsChecked(self, smoothFactor, maxDiff=1.0, fill=False, varBlock=False, thres=19.0):
        """Extension: both views (computeDisparityMapLeft / Right with these arguments) and the left-right check
        (disp12MaxDiff = maxDiff).  Returns (left_map, right_map) as float64; failed pixels are 0 or filled."""
        p = make_params(VIEW_LEFT, self.blockSize_, self.minDisparity_, self.maxDisparity_,
                        smoothFactor, self.cost, varBlock, thres, self.subpixel)
        return _ctx(self._context).search_lr(p, self.leftImage_, self.rightImage_, maxDiff, fill)

    def computeDisparityMapsCheckedSGM(self, P1, P2, paths=8, maxDiff=1.0, fill=False, uniquenessRatio=None, base="left"):
        """Extension: semi-global matching of the `base` view, the other view's map derived from the same sums, and
        the left-right check of the two (disp12MaxDiff = maxDiff) in one call.  Returns (left_map, right_map) as
        float64; failed pixels are 0 or filled.  uniquenessRatio: None, or the ratio test on the base winner."""
        if base not in ("left", "right"):
            raise ValueError("base must be 'left' or 'right'")
        p = make_params(VIEW_LEFT if base == "left" else VIEW_RIGHT, self.blockSize_, self.minDisparity_,
                        self.maxDisparity_, 1.0, self.cost, subpixel=self.subpixel)
        return _ctx(self._context).search_pair(p, self.leftImage_, self.rightImage_, (paths, P1, P2), uniquenessRatio,
                                               maxDiff, fill)


class LinearSearch:
    """Mirror of the reference's LinearSearch (LinearSearch.h:9-20)."""

    def __init__(self, leftImage, rightImage, context=None, search_range=200):
        self.leftImage, self.rightImage = leftImage, rightImage
        self._context, self._range = context, search_range

    def computeDisparityMap(self, smoothFactor):
        p = make_params(VIEW_LINEAR, 1, 0, self._range, smoothFactor, "ssd",
                        linear_range=self._range)
        return _ctx(self._context).search(p, self.leftImage, self.rightImage)


class ImageRectifier:
    """The boundary of the reference's ImageRectifier (rectification.hpp:50-66) once H_ and Hp_ are known: the
    rectifying homographies come from the caller (the reference estimates them from the fundamental matrix and the
    matches; that part is not on this path).  Rectification, search and the warp back run in one device call."""

    def __init__(self, left, right, H, Hp, context=None):
        self.leftImage_, self.rightImage_ = left, right
        self.H_ = np.asarray(H, dtype=np.float64).reshape(3, 3)
        self.Hp_ = np.asarray(Hp, dtype=np.float64).reshape(3, 3)
        self._context = context
        self.disparityMapLeft = self.disparityMapRight = None
        self._rect = None

    def _run(self, p):
        out, rl, rr = _ctx(self._context).search_unrectified(p, self.leftImage_, self.rightImage_, self.H_, self.Hp_,
                                                             rectified=True)
        self._rect = (rl, rr)
        return out

    def computeDisparityMapLeft(self, blockSize, minDisparity, maxDisparity, smoothFactor):
        self.disparityMapLeft = self._run(make_params(VIEW_LEFT, blockSize, minDisparity, maxDisparity, smoothFactor))

    def computeDisparityMapRight(self, blockSize, minDisparity, maxDisparity, smoothFactor, varBlock=False, thres=10.0):
        self.disparityMapRight = self._run(make_params(VIEW_RIGHT, blockSize, minDisparity, maxDisparity, smoothFactor,
                                                       var_block=varBlock, thres=thres))

    def getRectifiedLeft(self):
        """The rectified left image of the last compute call (rectification.cpp:499-501)."""
        return None if self._rect is None else self._rect[0]

    def getRectifiedRight(self):
        return None if self._rect is None else self._rect[1]

    def getDisparityMapLeft(self):
        return self.disparityMapLeft

    def getDisparityMapRight(self):
        return self.disparityMapRight


# ---- Middlebury plumbing (no GPU needed) -------------------------------------------------
def read_pfm(path):
    lib = load_library()
    data = ctypes.POINTER(ctypes.c_float)()
    w, h = ctypes.c_int(), ctypes.c_int()
    rc = lib.ws_pfm_read(os.fsencode(path), ctypes.byref(data), ctypes.byref(w), ctypes.byref(h))
    if rc != 0:
        raise WsError(rc, "cannot read PFM %s" % path)
    try:
        return np.ctypeslib.as_array(data, shape=(h.value, w.value)).copy()
    finally:
        lib.ws_free(data)


def write_pfm(path, array):
    a = np.ascontiguousarray(array, dtype=np.float32)
    rc = load_library().ws_pfm_write(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], a.shape[1])
    if rc != 0:
        raise WsError(rc, "cannot write PFM %s" % path)


def write_mesh_off(path, positions, colors, edge_threshold):
    pos = np.ascontiguousarray(positions, dtype=np.float32)
    col = np.ascontiguousarray(colors, dtype=np.uint8)
    h, w = pos.shape[:2]
    rc = load_library().ws_write_mesh_off(os.fsencode(path), pos.ctypes.data, col.ctypes.data, w, h, edge_threshold)
    if rc != 0:
        raise WsError(rc, "cannot write mesh %s" % path)


def read_ppm(path):
    """P6 file -> H x W x 3 uint8 in BGR order (what cv::imread(IMREAD_COLOR) would give)."""
    lib = load_library()
    data = ctypes.POINTER(ctypes.c_uint8)()
    w, h = ctypes.c_int(), ctypes.c_int()
    rc = lib.ws_ppm_read(os.fsencode(path), ctypes.byref(data), ctypes.byref(w), ctypes.byref(h))
    if rc != 0:
        raise WsError(rc, "cannot read PPM %s" % path)
    try:
        return np.ctypeslib.as_array(data, shape=(h.value, w.value, 3)).copy()
    finally:
        lib.ws_free(data)


def write_ppm(path, bgr):
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    rc = load_library().ws_ppm_write(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], a.strides[0])
    if rc != 0:
        raise WsError(rc, "cannot write PPM %s" % path)


def read_calib(path):
    c = _Calib()
    rc = load_library().ws_calib_read(os.fsencode(path), ctypes.byref(c))
    if rc != 0:
        raise WsError(rc, "cannot parse calib %s" % path)
    return {"cam0": np.array(c.cam0[:], dtype=np.float32).reshape(3, 3),
            "cam1": np.array(c.cam1[:], dtype=np.float32).reshape(3, 3),
            "doffs": c.doffs, "baseline": c.baseline, "width": c.width, "height": c.height,
            "ndisp": c.ndisp}


def evaldisp(disp, gt, mask, badthresh, maxdisp, rounddisp=0):
    d = np.ascontiguousarray(disp, dtype=np.float32)
    g = np.ascontiguousarray(gt, dtype=np.float32)
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if not (d.shape == g.shape == m.shape):
        raise ValueError("shape mismatch (the reference asserts, utils.cpp:128-129)")
    res = (ctypes.c_double * 6)()
    rc = load_library().ws_evaldisp(d.ctypes.data, g.ctypes.data, m.ctypes.data, d.shape[1],
                                    d.shape[0], badthresh, maxdisp, int(rounddisp), res)
    if rc != 0:
        raise WsError(rc, "evaldisp")
    return {"n": int(res[0]), "bad": res[1], "invalid": res[2], "total_bad": res[3],
            "avg_err": res[4], "valid": res[5]}
