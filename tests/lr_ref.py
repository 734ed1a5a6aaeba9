"""Plain NumPy statement of the left-right consistency check (include/ws_stereo.h, "left-right consistency check").

Test infrastructure only: the rules written out per pixel (the check, with NumPy doing a row's pixels at once) and per
row (the fill), in float32 like the device.  lr_check(left, right, max_diff, fill) -> (out_left, out_right, counts).
"""
import numpy as np

EMPTY, PASSED, FAILED = 0, 1, 2


def _check_map(a, b, s, max_diff):
    """States and outputs of map `a` against partner map `b`; s = -1 for the left map, +1 for the right map."""
    h, w = a.shape
    hb, wb = b.shape
    state = np.full((h, w), EMPTY, dtype=np.uint8)
    out = np.zeros((h, w), dtype=np.float32)
    x = np.arange(w, dtype=np.float64)
    md = np.float32(max_diff)
    for y in range(h):
        v = a[y]
        nonzero = v != 0                                   # rule 1: 0 and -0.0 are "no disparity"
        passed = np.zeros(w, dtype=bool)
        if y < hb:                                         # rule 2: no partner row -> fail
            finite = np.isfinite(v)
            d = np.rint(np.where(finite, v, 0)).astype(np.float64)   # half to even, like rintf
            p = x + s * d                                  # exact in double for every |d| < 2^53
            inside = finite & (p >= 0) & (p < wb)
            pi = np.where(inside, p, 0).astype(np.int64)
            with np.errstate(invalid="ignore", over="ignore"):
                diff = np.abs(v - b[y, pi])                # rule 3, float32 arithmetic
                passed = inside & (diff <= md)
        passed &= nonzero
        state[y] = np.where(passed, PASSED, np.where(nonzero, FAILED, EMPTY))
        out[y] = np.where(passed, v, np.float32(0))
    return state, out


def _fill_row(out_row, state_row):
    """Rule 4, WS_LR_FILL_BACKGROUND, on one output row: failed pixels from the nearest passed pixels left and right."""
    w = out_row.shape[0]
    x = np.arange(w)
    passed = state_row == PASSED
    left = np.maximum.accumulate(np.where(passed, x, -1))                    # nearest passed column <= x
    right = np.minimum.accumulate(np.where(passed, x, w)[::-1])[::-1]        # nearest passed column >= x
    has_l, has_r = left >= 0, right < w
    vl = out_row[np.clip(left, 0, w - 1)]
    vr = out_row[np.clip(right, 0, w - 1)]
    filled = np.where(has_l & has_r, np.fmin(vl, vr),               # both sides: the farther surface
                      np.where(has_l, vl, np.where(has_r, vr, np.float32(0))))   # one side, or none: 0
    return np.where(state_row == FAILED, filled, out_row).astype(np.float32)


def lr_states(left, right, max_diff):
    """(state_left, state_right): EMPTY / PASSED / FAILED per pixel."""
    left = np.asarray(left, dtype=np.float32)
    right = np.asarray(right, dtype=np.float32)
    return _check_map(left, right, -1.0, max_diff)[0], _check_map(right, left, 1.0, max_diff)[0]


def lr_check(left, right, max_diff=1.0, fill=False):
    """The checked maps (float32) and the failure counts (left, right) of two float32 maps (rule 5: filled pixels count)."""
    if not (max_diff >= 0):
        raise ValueError("max_diff must be >= 0 and not NaN")
    left = np.asarray(left, dtype=np.float32)
    right = np.asarray(right, dtype=np.float32)
    outs, counts = [], []
    for a, b, s in ((left, right, -1.0), (right, left, 1.0)):
        state, out = _check_map(a, b, s, max_diff)
        if fill:
            out = np.stack([_fill_row(out[y], state[y]) for y in range(out.shape[0])]) if out.shape[0] else out
        outs.append(out)
        counts.append(int(np.count_nonzero(state == FAILED)))
    return outs[0], outs[1], tuple(counts)
