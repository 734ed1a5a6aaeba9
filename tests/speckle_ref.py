"""Two independent statements of the speckle filter (include/ws_stereo.h, "speckle filter"), test infrastructure only.

The rules, restated: for a float32 map A and (new_val, max_speckle_size, max_diff),
  1. a pixel is blank if A == new_val (float ==, so -0.0 is blank for new_val 0); blank pixels belong to no region and
     keep their bits;
  2. two 4-neighbours join if neither is blank and fabsf(a - b) <= max_diff in float32 (NaN joins nothing; +inf joins
     only with max_diff = +inf, and never another +inf);
  3. a region is a connected component of those joins;
  4. every pixel of a region of count <= max_speckle_size becomes exactly new_val, every other pixel keeps its bits;
  5. counts: (pixels set to new_val, regions removed);
  6. refused: new_val NaN, max_diff NaN or negative, max_speckle_size < 0, an empty map.

filter_speckles_wavefront: OpenCV's filterSpecklesImpl loop (calib3d/src/stereosgbm.cpp) written out literally -- labels,
a stack, rtype -- in float32; pure Python, for small maps.
filter_speckles: the components of the join graph from scipy.sparse.csgraph.connected_components, vectorised, for maps
of any size.
Both return (filtered float32 map, (pixels set, regions removed)).
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def _check(a, new_val, max_speckle_size, max_diff):
    a = np.array(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("expected a non-empty H x W map")
    if np.isnan(np.float32(new_val)):
        raise ValueError("new_val is NaN")
    if not (max_diff >= 0):
        raise ValueError("max_diff must be >= 0 and not NaN")
    if max_speckle_size < 0:
        raise ValueError("max_speckle_size must be >= 0")
    return a, np.float32(new_val), int(max_speckle_size), np.float32(max_diff)


def filter_speckles_wavefront(img, new_val=0.0, max_speckle_size=100, max_diff=1.0):
    a, nv, max_size, md = _check(img, new_val, max_speckle_size, max_diff)
    h, w = a.shape
    labels = np.zeros((h, w), dtype=np.int64)
    rtype = [0]
    curlabel = 0
    pixels = regions = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(h):
            for j in range(w):
                if a[i, j] != nv:
                    if labels[i, j]:
                        if rtype[labels[i, j]]:
                            a[i, j] = nv
                            pixels += 1
                    else:
                        curlabel += 1
                        rtype.append(0)
                        ws = [(i, j)]
                        labels[i, j] = curlabel
                        count = 0
                        while ws:
                            y, x = ws.pop()
                            count += 1
                            dp = a[y, x]
                            # OpenCV's order: below, above, right, left
                            for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                                if 0 <= yy < h and 0 <= xx < w and labels[yy, xx] == 0:
                                    dpp = a[yy, xx]
                                    if dpp != nv and np.abs(dp - dpp) <= md:
                                        labels[yy, xx] = curlabel
                                        ws.append((yy, xx))
                        if count <= max_size:
                            rtype[curlabel] = 1
                            a[i, j] = nv
                            pixels += 1
                            regions += 1
    return a, (pixels, regions)


def join_edges(a, nv, md):
    """(from, to) flat indices of every join (rule 2) between horizontal and vertical neighbours."""
    h, w = a.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    keep = a != nv
    with np.errstate(invalid="ignore", over="ignore"):
        jh = keep[:, :-1] & keep[:, 1:] & (np.abs(a[:, :-1] - a[:, 1:]) <= md)
        jv = keep[:-1, :] & keep[1:, :] & (np.abs(a[:-1, :] - a[1:, :]) <= md)
    return (np.concatenate([idx[:, :-1][jh], idx[:-1, :][jv]]), np.concatenate([idx[:, 1:][jh], idx[1:, :][jv]]))


def regions(img, new_val=0.0, max_diff=1.0):
    """(component label per pixel, size per component counted over non-blank pixels, non-blank mask), flat."""
    a, nv, _, md = _check(img, new_val, 0, max_diff)
    n = a.size
    src, dst = join_edges(a, nv, md)
    graph = coo_matrix((np.ones(src.size, dtype=np.int8), (src, dst)), shape=(n, n))
    _, lab = connected_components(graph, directed=False)
    keep = (a != nv).reshape(-1)
    sizes = np.bincount(lab[keep], minlength=lab.max() + 1)
    return lab, sizes, keep


def filter_speckles(img, new_val=0.0, max_speckle_size=100, max_diff=1.0):
    a, nv, max_size, md = _check(img, new_val, max_speckle_size, max_diff)
    lab, sizes, keep = regions(a, nv, md)
    small = (sizes > 0) & (sizes <= max_size)
    remove = keep & small[lab]
    out = a.reshape(-1).copy()
    out[remove] = nv
    return out.reshape(a.shape), (int(np.count_nonzero(remove)), int(np.count_nonzero(small)))


# ---- maps shared by the CPU and device tests ------------------------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 2.0, 2.5, -1.0, 1e30], dtype=np.float32)


def random_map(rng, h, w, levels=6, special=0.2, scale=1.0):
    """Integer levels (ties everywhere) scaled by `scale`, with a fraction of special values mixed in."""
    a = (rng.integers(0, levels, size=(h, w)) * scale).astype(np.float32)
    mask = rng.random((h, w)) < special
    a[mask] = rng.choice(SPECIAL, size=int(mask.sum()))
    return a


def serpentine(h, w, val=5.0, segment=0):
    """A one-pixel-wide path on a blank (0) background: full rows at every even y, joined by one pixel at alternating
    ends of the odd rows.  One region that crosses every tile; with segment > 0 the value steps by 10 every `segment`
    pixels along the path instead, which cuts it into regions of `segment` pixels."""
    a = np.zeros((h, w), dtype=np.float32)
    ys, xs = [], []
    for y in range(h):
        if y % 2 == 0:
            x = np.arange(w) if (y // 2) % 2 == 0 else np.arange(w - 1, -1, -1)
        else:
            x = np.array([w - 1 if (y // 2) % 2 == 0 else 0])
        ys.append(np.full(x.size, y))
        xs.append(x)
    ys, xs = np.concatenate(ys), np.concatenate(xs)
    s = np.arange(ys.size)
    a[ys, xs] = val if segment <= 0 else (10 * (s // segment) + 1).astype(np.float32)
    return a


def spiral(h, w, val=5.0):
    """A one-pixel-wide square spiral walled by blank (0) pixels, from the outer ring inwards."""
    a = np.zeros((h, w), dtype=np.float32)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    start = 0  # the column the ring's top row starts from (the previous ring's left column joins it there)
    while top <= bottom and left <= right:
        a[top, start:right + 1] = val
        a[top:bottom + 1, right] = val
        if bottom - top >= 2:
            a[bottom, left:right + 1] = val
            if right - left >= 2:
                a[top + 2:bottom + 1, left] = val
        start = left
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return a


def checkerboard(h, w):
    """Non-blank pixels only where x + y is even, so every one is a region of its own."""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, ((7 * x + 13 * y) % 50 + 1).astype(np.float32), np.float32(0)).astype(np.float32)
