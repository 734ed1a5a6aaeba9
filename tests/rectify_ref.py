"""CPU restatement of the rectification half of ImageRectifier (rectification.cpp:432-493): the size of a rectified
image, and cv::warpPerspective(img, dst, H, size) with INTER_LINEAR, BORDER_CONSTANT 0 on CV_8UC3.

OpenCV is not vendored by the reference.  This restates OpenCV 4.x's fixed-point bilinear path (the one OpenCV <= 4.10
runs on x86: WarpPerspectiveInvoker + remapBilinear, INTER_BITS 5, INTER_REMAP_COEF_BITS 15).  PARITY UNPINNED: later
OpenCV releases may differ by one grey level.

Two independent forms:
  * warp_linear_u8: vectorised NumPy, used at full size;
  * warp_linear_u8_loop: a plain per-pixel loop over OpenCV's column blocks, written separately as the witness for the
    NumPy form (tests/test_rectify_reference.py compares the two).
"""
import math

import numpy as np

FLT_EPSILON = 1.1920928955078125e-07
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def inv3(m):
    """3x3 inverse by adjugate / determinant (the closed form cv::invert uses for 3x3, ws_capi.cpp invert3x3)."""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)]
    d = (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])
         + m[2] * (m[3] * m[7] - m[4] * m[6]))
    if d == 0.0:
        raise ZeroDivisionError("singular matrix")
    r = 1.0 / d
    return np.array([(m[4] * m[8] - m[5] * m[7]) * r, (m[2] * m[7] - m[1] * m[8]) * r, (m[1] * m[5] - m[2] * m[4]) * r,
                     (m[5] * m[6] - m[3] * m[8]) * r, (m[0] * m[8] - m[2] * m[6]) * r, (m[2] * m[3] - m[0] * m[5]) * r,
                     (m[3] * m[7] - m[4] * m[6]) * r, (m[1] * m[6] - m[0] * m[7]) * r, (m[0] * m[4] - m[1] * m[3]) * r])


def rectified_size(H, w, h):
    """(cols, rows) of rectification.cpp:436-483, or None where ws_rectified_size returns WS_ERR_GEOMETRY."""
    m = [float(v) for v in np.asarray(H, dtype=np.float64).reshape(9)]
    xs, ys = [], []
    for x, y in ((0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h))):
        wq = x * m[6] + y * m[7] + m[8]
        if not abs(wq) > FLT_EPSILON:
            return None
        wq = 1.0 / wq
        xs.append((x * m[0] + y * m[1] + m[2]) * wq)
        ys.append((x * m[3] + y * m[4] + m[5]) * wq)
    cols, rows = max(xs) - min(xs), max(ys) - min(ys)
    if not (1.0 <= cols < 32768.0 and 1.0 <= rows < 32768.0):
        return None
    return int(cols), int(rows)


def block_width(dst_w, dst_h):
    """OpenCV's column block: bw0 = min(BLOCK_SZ^2 / min(BLOCK_SZ/2, rows), cols), BLOCK_SZ = 32."""
    return min(1024 // min(16, dst_h), dst_w)


def _clamp_int(v):
    """max(INT_MIN, min(INT_MAX, v)) as std::min / std::max evaluate it: a NaN (0 * inf, where 32 / W overflowed for a
    subnormal W) becomes INT_MAX, not whatever np.clip and a cast to int would make of it."""
    return np.clip(np.where(np.isnan(v), INT_MAX, v), INT_MIN, INT_MAX)


def warp_linear_u8(src, H, dst_shape, rows_per_chunk=256):
    """cv::warpPerspective(src, dst, H, (dst_shape[1], dst_shape[0])), INTER_LINEAR, BORDER_CONSTANT 0, uint8 x 3."""
    src = np.asarray(src, dtype=np.uint8)
    sh, sw = src.shape[:2]
    dh, dw = dst_shape
    m = inv3(H)
    out = np.zeros((dh, dw, 3), dtype=np.uint8)
    bw0 = block_width(dw, dh)
    xs = np.arange(dw)
    x1 = (xs % bw0).astype(np.float64)
    xb = (xs - xs % bw0).astype(np.float64)
    flat = src.astype(np.int64)
    for y0 in range(0, dh, rows_per_chunk):
        y = np.arange(y0, min(dh, y0 + rows_per_chunk), dtype=np.float64)[:, None]
        X0 = m[0] * xb + m[1] * y + m[2]
        Y0 = m[3] * xb + m[4] * y + m[5]
        W = m[6] * xb + m[7] * y + m[8] + m[6] * x1
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            W = np.where(W != 0, 32.0 / np.where(W != 0, W, 1.0), 0.0)
            fx = _clamp_int((X0 + m[0] * x1) * W)
            fy = _clamp_int((Y0 + m[3] * x1) * W)
        X = np.rint(fx).astype(np.int64)
        Y = np.rint(fy).astype(np.int64)
        sx = np.clip(X >> 5, -32768, 32767)
        sy = np.clip(Y >> 5, -32768, 32767)
        ax, ay = X & 31, Y & 31
        acc = np.full(X.shape + (3,), 16384, dtype=np.int64)
        for dy, dx, wt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32),
                           (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
            tx, ty = sx + dx, sy + dy
            inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
            v = flat[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)]
            acc += np.where(inside, wt, 0)[..., None] * v
        out[y0:y0 + X.shape[0]] = (acc >> 15).astype(np.uint8)
    return out


def warp_linear_u8_loop(src, H, dst_shape):
    """The witness: WarpPerspectiveInvoker's block loop and remapBilinear's taps, one pixel at a time, in Python floats."""
    src = np.asarray(src, dtype=np.uint8)
    sh, sw = src.shape[:2]
    dh, dw = dst_shape
    M = [float(v) for v in inv3(H)]
    out = np.zeros((dh, dw, 3), dtype=np.uint8)
    bw0 = block_width(dw, dh)

    def sat16(v):
        return max(-32768, min(32767, v))

    def pix(x, y, c):
        return int(src[y, x, c]) if 0 <= x < sw and 0 <= y < sh else 0

    for y in range(dh):
        for x in range(0, dw, bw0):
            X0 = M[0] * x + M[1] * y + M[2]
            Y0 = M[3] * x + M[4] * y + M[5]
            W0 = M[6] * x + M[7] * y + M[8]
            for x1 in range(min(bw0, dw - x)):
                W = W0 + M[6] * x1
                W = 32.0 / W if W != 0 else 0.0
                fX = max(INT_MIN, min(INT_MAX, (X0 + M[0] * x1) * W))
                fY = max(INT_MIN, min(INT_MAX, (Y0 + M[3] * x1) * W))
                X, Y = int(round(fX)), int(round(fY))  # Python's round(): half to even, like cvRound
                sx, sy = sat16(X >> 5), sat16(Y >> 5)
                a, b = X & 31, Y & 31
                for c in range(3):
                    s = (pix(sx, sy, c) * (32 - a) * (32 - b) * 32 + pix(sx + 1, sy, c) * a * (32 - b) * 32
                         + pix(sx, sy + 1, c) * (32 - a) * b * 32 + pix(sx + 1, sy + 1, c) * a * b * 32)
                    out[y, x + x1, c] = (s + 16384) >> 15
    return out


def rectifying_homography(w, h, angle_deg=1.5, shear=0.01, persp=(2e-5, -1e-5), scale=1.0, shift=(8.0, -5.0)):
    """A rectifying-looking H (small rotation, shear, perspective), centred on the image."""
    a = math.radians(angle_deg)
    cx, cy = w / 2.0, h / 2.0
    T = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]], dtype=np.float64)
    R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    S = np.array([[scale, shear, 0], [0, scale, 0], [0, 0, 1]])
    P = np.array([[1, 0, 0], [0, 1, 0], [persp[0], persp[1], 1]])
    B = np.array([[1, 0, cx + shift[0]], [0, 1, cy + shift[1]], [0, 0, 1]])
    return B @ S @ R @ P @ T
