"""CPU checks of the rectification restatement (tests/rectify_ref.py) and of ws_rectified_size (host only, no device).

The NumPy warp is what the GPU tests compare the device against; here it is held to a per-pixel witness written
separately, and to known answers that need neither."""
import ctypes
import zlib

import numpy as np
import pytest

import rectify_ref as rr

# (name, H builder taking (src_w, src_h)) -- dst sizes are chosen per case
CASES = [
    ("identity", lambda w, h: np.eye(3)),
    ("near_identity_rectifying", lambda w, h: rr.rectifying_homography(w, h, 0.7, 0.004, (3e-4, -2e-4), 1.0, (1.3, -0.6))),
    ("strong_perspective", lambda w, h: np.array([[0.9, 0.12, 2.0], [-0.05, 1.1, 1.0], [4e-3, -3e-3, 1.0]])),
    ("rotation_30", lambda w, h: rr.rectifying_homography(w, h, 30.0, 0.0, (0.0, 0.0), 1.0, (0.0, 0.0))),
    ("upscale", lambda w, h: np.array([[2.37, 0.0, -3.1], [0.0, 1.71, -1.4], [0.0, 0.0, 1.0]])),
    ("downscale", lambda w, h: np.array([[0.41, 0.03, 0.7], [0.0, 0.55, 0.2], [0.0, 0.0, 1.0]])),
    ("partly_outside", lambda w, h: np.array([[1.0, 0.0, w * 0.4], [0.0, 1.0, -h * 0.3], [0.0, 0.0, 1.0]])),
    ("fully_outside", lambda w, h: np.array([[1.0, 0.0, 5.0 * w], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])),
    ("negative_w_region", lambda w, h: np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-0.05, 0.0, 1.0]])),
]

SHAPES = [  # (src_h, src_w, dst_h, dst_w): below / at / above the 64-column block, fewer than 16 rows, 1x1
    (23, 37, 21, 41),
    (19, 70, 17, 65),
    (12, 30, 5, 130),   # 5 rows: bw0 = min(1024 // 5, 130) = 130, one block per row
    (40, 33, 15, 90),   # 15 rows: bw0 = 68
    (1, 1, 1, 1),
    (9, 9, 3, 3),
]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_numpy_restatement_equals_the_per_pixel_witness(name, make, shape):
    sh, sw, dh, dw = shape
    rng = np.random.default_rng(zlib.crc32(repr((name, shape)).encode()))
    src = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    H = make(sw, sh)
    a = rr.warp_linear_u8(src, H, (dh, dw))
    b = rr.warp_linear_u8_loop(src, H, (dh, dw))
    assert np.array_equal(a, b), (name, shape, np.argwhere(a != b)[:5])


def test_numpy_restatement_equals_the_witness_under_random_homographies():
    rng = np.random.default_rng(5)
    for k in range(12):
        sh, sw = int(rng.integers(1, 30)), int(rng.integers(1, 80))
        dh, dw = int(rng.integers(1, 30)), int(rng.integers(1, 140))
        H = np.eye(3) + rng.normal(0, [[0.2, 0.2, 3.0], [0.2, 0.2, 3.0], [0.01, 0.01, 0.0]])
        src = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
        a = rr.warp_linear_u8(src, H, (dh, dw), rows_per_chunk=7)  # (and across row chunks)
        b = rr.warp_linear_u8_loop(src, H, (dh, dw))
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:5])


def test_subnormal_w_overflows_to_nan_and_clamps_to_int_max():
    """inv(H)[8] = 1e-308 is subnormal: 32 / W overflows to inf, 0 * inf is NaN at column 0, and
    max(INT_MIN, min(INT_MAX, NaN)) is INT_MAX in C++ (std::min / std::max, the kernel's fmin / fmax) and in Python's
    min / max.  Both restatements take every tap outside the source."""
    H = np.diag([1.0, 1.0, 1e308])
    assert 0.0 < rr.inv3(H)[8] < 2.2250738585072014e-308
    assert rr._clamp_int(np.array([np.nan, np.inf, -np.inf, 3.5])).tolist() == [rr.INT_MAX, rr.INT_MAX, rr.INT_MIN, 3.5]
    src = np.random.default_rng(6).integers(1, 256, size=(9, 40, 3), dtype=np.uint8)
    a = rr.warp_linear_u8(src, H, (6, 70))
    assert np.array_equal(a, rr.warp_linear_u8_loop(src, H, (6, 70)))
    assert not a.any()


def test_identity_is_an_exact_copy():
    src = np.random.default_rng(1).integers(0, 256, size=(37, 101, 3), dtype=np.uint8)
    assert np.array_equal(rr.warp_linear_u8(src, np.eye(3), src.shape[:2]), src)


@pytest.mark.parametrize("tx,ty", [(3, 0), (-5, 2), (0, -4), (70, 1)])
def test_integer_translation_is_a_shifted_copy_with_zeros(tx, ty):
    src = np.random.default_rng(2).integers(1, 256, size=(30, 90, 3), dtype=np.uint8)
    H = np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
    want = np.zeros_like(src)
    h, w = src.shape[:2]
    for y in range(h):
        for x in range(w):
            if 0 <= x - tx < w and 0 <= y - ty < h:
                want[y, x] = src[y - ty, x - tx]
    assert np.array_equal(rr.warp_linear_u8(src, H, (h, w)), want)


def test_half_pixel_shift_averages_neighbours_with_rounding():
    src = np.random.default_rng(3).integers(0, 256, size=(20, 77, 3), dtype=np.uint8)
    H = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    got = rr.warp_linear_u8(src, H, src.shape[:2]).astype(np.int32)
    s = src.astype(np.int32)
    assert np.array_equal(got[:, 1:], (s[:, :-1] + s[:, 1:] + 1) >> 1)
    assert np.array_equal(got[:, 0], (s[:, 0] + 1) >> 1)


def test_block_width_follows_opencv():
    assert rr.block_width(3840, 2160) == 64
    assert rr.block_width(40, 2160) == 40
    assert rr.block_width(1000, 5) == 204
    assert rr.block_width(1, 1) == 1


# ---- ws_rectified_size (host only) ----------------------------------------------------------------------------------

def _lib_size(wslib, H, w, h):
    lib = wslib.load_library()
    m = (ctypes.c_double * 9)(*np.asarray(H, dtype=np.float64).reshape(9))
    ow, oh = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.ws_rectified_size(m, w, h, ctypes.byref(ow), ctypes.byref(oh))
    return rc, (ow.value, oh.value)


def test_rectified_size_matches_the_restatement(wslib):
    rng = np.random.default_rng(9)
    Hs = [np.eye(3), rr.rectifying_homography(1500, 1000), rr.rectifying_homography(900, 750, -2.0, 0.02, (1e-4, 5e-5), 1.1),
          np.array([[1.0, 0.0, -300.0], [0.0, 1.0, 40.0], [0.0, 0.0, 1.0]])]
    Hs += [np.eye(3) + rng.normal(0, [[0.1, 0.1, 20.0], [0.1, 0.1, 20.0], [1e-4, 1e-4, 0.0]]) for _ in range(40)]
    for H in Hs:
        for w, h in ((1500, 1000), (900, 750), (64, 15), (1, 1), (3840, 2160)):
            want = rr.rectified_size(H, w, h)
            rc, got = _lib_size(wslib, H, w, h)
            if want is None:
                assert rc == -2, (H, w, h)
            else:
                assert rc == 0 and got == want, (H, w, h, got, want)


def test_rectified_size_of_the_identity_and_a_translation_is_the_image_size(wslib):
    assert _lib_size(wslib, np.eye(3), 1500, 1000) == (0, (1500, 1000))
    # not translated by min_x / min_y: the extent stays the image's (rectification.cpp:476-483)
    assert _lib_size(wslib, [[1, 0, -40.5], [0, 1, 7.25], [0, 0, 1]], 640, 480) == (0, (640, 480))
    assert wslib.rectified_size(np.eye(3), (480, 640, 3)) == (480, 640)


def test_rectified_size_truncates(wslib):
    H = np.diag([1.0049, 0.9951, 1.0])
    assert _lib_size(wslib, H, 1000, 1000) == (0, (1004, 995)) == (0, rr.rectified_size(H, 1000, 1000))


@pytest.mark.parametrize("H,w,h", [
    ([[1, 0, 0], [0, 1, 0], [0, 0, 0]], 10, 10),               # w = 0 at corner (0,0)
    ([[1, 0, 0], [0, 1, 0], [-0.01, 0, 1]], 100, 10),          # w = 0 at the right corners
    ([[1, 0, 0], [0, 1, 0], [0, 0, 1e-9]], 10, 10),            # |w| <= FLT_EPSILON
    ([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]], 1, 1),             # 0 x 0
    ([[40.0, 0, 0], [0, 1, 0], [0, 0, 1]], 1000, 10),         # 40000 columns
    ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], 32768, 2),            # 32768 columns
])
def test_rectified_size_geometry_errors(wslib, H, w, h):
    assert rr.rectified_size(H, w, h) is None
    assert _lib_size(wslib, H, w, h)[0] == -2
    with pytest.raises(wslib.WsError) as e:
        wslib.rectified_size(H, (h, w))
    assert e.value.code == -2


def test_rectified_size_largest_accepted(wslib):
    assert _lib_size(wslib, np.eye(3), 32767, 32767) == (0, (32767, 32767))


def test_rectified_size_argument_errors(wslib):
    lib = wslib.load_library()
    ow, oh = ctypes.c_int(), ctypes.c_int()
    m = (ctypes.c_double * 9)(*np.eye(3).reshape(9))
    assert lib.ws_rectified_size(None, 10, 10, ctypes.byref(ow), ctypes.byref(oh)) == -1
    assert lib.ws_rectified_size(m, 0, 10, ctypes.byref(ow), ctypes.byref(oh)) == -1
    assert lib.ws_rectified_size(m, 10, 10, None, ctypes.byref(oh)) == -1
