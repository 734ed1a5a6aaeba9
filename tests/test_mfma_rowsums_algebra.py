"""The row sums of the matrix-core SSD kernel (csrc/ws_march_mfma.h) as a 7-pixel box over per-pixel sums, in NumPy.

The kernel needs, for every target centre v of a tile row, the sum of squares and the sum of the 21 centred bytes
b^ = b - 128 of the row of its window.  It forms them per PIXEL -- one lane, one pixel: q = sum of the 3 squares,
r = sum of the 3 RAW bytes, packed as w = (q << 13) + r -- and adds the words of 7 consecutive pixels in a chunk of 64
lanes with six wave shifts (lane i takes lane i + 1's value, lane 63 takes 0): s <- w + shift(s), six times.  Lanes
0 .. 57 of a chunk then hold whole windows and own their centres; chunk c starts at pixel min(58 c, 326), so 7 chunks
cover the 384 centres (the eighth wave runs the last chunk again), and where two chunks overlap both owners hold the
same words.  The unpacked fields give Q = s >> 13 and T = (s & 8191) - 2688.

This file restates that arithmetic with the kernel's constants and compares it with the per-centre dot sums it
replaces, exactly: random rows, rows of all 0 and all 255, rows alternating per byte and per pixel, every byte phase
0 .. 15 of the row's start; the fields' bounds, met with equality at the extremes; the chunk edges.
"""
import numpy as np
import pytest

WW = 7                 # window columns
K = 3 * WW             # window bytes per row
NVC = 384              # target centres per tile row: 128 columns + 8 x 32 candidates
NPIX = NVC + 12        # pixels per raw row the copies fetch
LANES = 64
CW = LANES - (WW - 1)  # centres a chunk of 64 pixels yields: 58
SHIFT = 13             # the square sums sit above the raw byte sums
NCHUNK = -(-NVC // CW)


def chunk_start(c):
    return min(CW * c, NVC - CW)


def raw_buffer(row_bytes, phase):
    """The raw row as it lies in LDS: its first byte at offset `phase` of a 16-byte aligned buffer, zeros around it."""
    buf = np.zeros(16 + len(row_bytes) + 32, dtype=np.uint8)
    buf[phase:phase + len(row_bytes)] = row_bytes
    return buf


def pixel_words(buf, phase, p0):
    """The packed words of pixels p0 .. p0 + 63: two aligned dwords, one byte alignment, centre and mask, two dots."""
    at = phase + 3 * (p0 + np.arange(LANES))
    lo = at & ~3
    sh = at & 3
    # (dwords past the buffer's end read as zeros, like the ring bytes outside the image)
    ext = np.concatenate([buf, np.zeros(256, dtype=np.uint8)])
    d = np.stack([ext[lo + k].astype(np.uint64) for k in range(8)], axis=1)
    d0 = d[:, 0] | d[:, 1] << 8 | d[:, 2] << 16 | d[:, 3] << 24
    d1 = d[:, 4] | d[:, 5] << 8 | d[:, 6] << 16 | d[:, 7] << 24
    x = (((d1 << 32) | d0) >> (8 * sh.astype(np.uint64))) & np.uint64(0xffffffff)     # v_alignbyte
    cm = (x ^ np.uint64(0x00808080)) & np.uint64(0x00ffffff)                           # centred, the 4th byte masked
    by = np.stack([(cm >> np.uint64(8 * k)) & np.uint64(0xff) for k in range(3)], axis=1).astype(np.int64)
    by = np.where(by >= 128, by - 256, by)                                             # read as signed bytes
    q = (by * by).sum(axis=1)
    raw = np.stack([(x >> np.uint64(8 * k)) & np.uint64(0xff) for k in range(3)], axis=1).astype(np.int64)
    r = raw.sum(axis=1)
    assert q.max() <= 3 * 128 * 128 and r.max() <= 3 * 255
    return ((q << SHIFT) + r).astype(np.uint32)


def above(v):
    """wave_shl:1 -- lane i takes lane i + 1's value, lane 63 takes 0."""
    return np.concatenate([v[1:], np.zeros(1, dtype=np.uint32)])


def box(w):
    """s <- w + above(s), WW - 1 times, in 32-bit words."""
    s = w.copy()
    for _ in range(WW - 1):
        s = (w + above(s)).astype(np.uint32)
    return s


def row_sums_by_chunks(row_bytes, phase):
    """(Q[NVC], T[NVC], the packed window words) as the chunks' owners produce them."""
    buf = raw_buffer(row_bytes, phase)
    Q = np.full(NVC, -1, dtype=np.int64)
    T = np.full(NVC, -1, dtype=np.int64)
    S = np.zeros(NVC, dtype=np.uint32)
    owners = np.zeros(NVC, dtype=np.int64)
    for c in range(NCHUNK + 1):              # (the eighth wave's chunk starts where the seventh's does)
        p0 = chunk_start(c)
        s = box(pixel_words(buf, phase, p0))
        own = np.arange(LANES) < CW
        v, s = p0 + np.arange(LANES)[own], s[own]
        assert v.max() < NVC
        seen = owners[v] > 0
        assert np.array_equal(S[v][seen], s[seen]), "two owners of a centre hold the same word"
        Q[v] = (s >> SHIFT).astype(np.int64)
        T[v] = (s & np.uint32((1 << SHIFT) - 1)).astype(np.int64) - 128 * K
        S[v] = s
        owners[v] += 1
    assert (owners >= 1).all(), "every centre has an owner"
    assert (owners[:chunk_start(NCHUNK - 1)] == 1).all() and (owners[CW * (NCHUNK - 1):] == 2).all()
    return Q, T, S


def row_sums_direct(row_bytes):
    """Per centre: the dots over its 21 window bytes, centred (what the lane pairs formed)."""
    b = row_bytes.astype(np.int64) - 128
    idx = 3 * np.arange(NVC)[:, None] + np.arange(K)[None, :]
    win = b[idx]
    return (win * win).sum(axis=1), win.sum(axis=1)


def rows():
    rng = np.random.default_rng(5)
    n = 3 * NPIX
    out = {"random_%d" % k: rng.integers(0, 256, n, dtype=np.uint8) for k in range(3)}
    out["all_0"] = np.zeros(n, dtype=np.uint8)
    out["all_255"] = np.full(n, 255, dtype=np.uint8)
    out["bytes_0_255"] = np.where(np.arange(n) % 2 == 0, 0, 255).astype(np.uint8)
    out["bytes_255_0"] = np.where(np.arange(n) % 2 == 0, 255, 0).astype(np.uint8)
    out["pixels_0_255"] = np.where((np.arange(n) // 3) % 2 == 0, 0, 255).astype(np.uint8)
    out["pixels_255_0"] = np.where((np.arange(n) // 3) % 2 == 0, 255, 0).astype(np.uint8)
    out["all_128"] = np.full(n, 128, dtype=np.uint8)
    return out


ROWS = rows()


@pytest.mark.parametrize("phase", range(16))
@pytest.mark.parametrize("name", sorted(ROWS))
def test_box_of_pixel_words_is_the_window_dot(name, phase):
    row = ROWS[name]
    Q, T, _ = row_sums_by_chunks(row, phase)
    q, t = row_sums_direct(row)
    assert np.array_equal(Q, q)
    assert np.array_equal(T, t)


def test_fields_meet_their_bounds_and_never_borrow():
    # square sums: largest for bytes 0 (centred -128), window 21 x 128^2 = 344064 < 2^19; zero for bytes 128
    Q, T, S = row_sums_by_chunks(ROWS["all_0"], 3)
    assert (Q == K * 128 * 128).all() and K * 128 * 128 == 344064 < 1 << 19
    assert (T == -128 * K).all() and (S & np.uint32(8191) == 0).all()
    Q, T, S = row_sums_by_chunks(ROWS["all_128"], 3)
    assert (Q == 0).all() and (S >> SHIFT == 0).all() and (T == 0).all()
    # raw byte sums: largest for bytes 255, 21 x 255 = 5355 < 2^13: the field is full to its bound and the squares above
    # it are exactly 21 x 127^2 -- nothing crossed
    Q, T, S = row_sums_by_chunks(ROWS["all_255"], 3)
    assert ((S & np.uint32(8191)) == K * 255).all() and K * 255 == 5355 < 1 << SHIFT
    assert (Q == K * 127 * 127).all() and (T == K * 127).all()
    # both fields at their largest together fit the word
    assert (K * 128 * 128 << SHIFT) + K * 255 < 1 << 32
    assert 19 + SHIFT == 32
    # the last lanes of a chunk (58 .. 63: windows cut short by the shift's zeros) stay inside their fields too
    for name in ("all_0", "all_255"):
        s = box(pixel_words(raw_buffer(ROWS[name], 0), 0, 0))
        assert ((s & np.uint32(8191)) <= K * 255).all() and ((s >> SHIFT) <= K * 128 * 128).all()


def test_chunk_edges():
    starts = [chunk_start(c) for c in range(NCHUNK)]
    assert NCHUNK == 7 and starts == [0, 58, 116, 174, 232, 290, 326] and chunk_start(NCHUNK) == starts[-1]
    # every chunk's pixels lie inside the raw row the copies fetch
    assert max(starts) + LANES <= NPIX
    # a centre whose window straddles a chunk boundary (pixels 52 .. 63 of chunk 0 are pixels of chunk 1's windows too)
    rng = np.random.default_rng(9)
    row = rng.integers(0, 256, 3 * NPIX, dtype=np.uint8)
    Q, T, _ = row_sums_by_chunks(row, 11)
    q, t = row_sums_direct(row)
    for c in range(1, NCHUNK):
        for v in range(CW * c - WW, CW * c + WW):
            assert Q[v] == q[v] and T[v] == t[v], (c, v)
    # the last chunk starts inside the one before it and owns only what that one does not
    assert np.array_equal(Q[NVC - WW:], q[NVC - WW:]) and np.array_equal(T[NVC - WW:], t[NVC - WW:])
    # a change of one byte moves exactly the 7 centres whose windows hold its pixel
    row2 = row.copy()
    row2[3 * 200 + 1] ^= 0x55
    Q2, T2, _ = row_sums_by_chunks(row2, 11)
    moved = np.flatnonzero((Q2 != Q) | (T2 != T))
    assert set(moved) <= set(range(200 - WW + 1, 201)) and len(moved) >= 1


def test_running_sum_is_the_lane_pairs():
    """gsum += Q + 2 T of the entering row - Q of the leaving row, modulo 2^32, against the window sums formed directly."""
    rng = np.random.default_rng(13)
    img = rng.integers(0, 256, (20, 3 * NPIX), dtype=np.uint8)
    img[5] = 0
    img[6] = 255
    WH = 7
    g = np.zeros(NVC, dtype=np.uint32)
    stash = []
    for y in range(img.shape[0]):
        Q, T, _ = row_sums_by_chunks(img[y], (5 * y) % 16)
        u = (Q + 2 * T).astype(np.int64)
        if y >= WH:
            u = u - stash[y - WH]
        stash.append(Q)
        g = (g.astype(np.int64) + u).astype(np.uint32)
        lo = max(0, y - WH + 1)
        want = sum(row_sums_direct(img[r])[0] for r in range(lo, y + 1)) + 2 * sum(row_sums_direct(img[r])[1] for r in range(y + 1))
        assert np.array_equal(g, want.astype(np.uint32))
