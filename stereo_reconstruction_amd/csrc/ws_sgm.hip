// ws_sgm.hip -- semi-global matching (extension; the rules are in include/ws_stereo.h).  Integer work only, no MFMA.
//   * ws_sgm_kr_kernel: one lane per pixel of the map.  The pixel's candidate interval [lo, hi) of disparity indices
//     (closed form from the geometry), or the two non-node kinds: no candidate (the fallback) and black / outside (0).
//   * ws_sgm_cost_kernel: the window costs C(p, j) of 64 columns x 64 disparities x kSgmStrip rows per workgroup, j
//     innermost in memory.  Each lane keeps the column sums of its disparity for a quarter of the tile's columns (plus
//     the window's halo) in registers and slides them down the strip: two pixel costs per column and row once the
//     window is full.  The sums go through LDS; each wave then slides the window along 16 columns.  Exact integers, in
//     16 bits where the host's bound allows.
//   * ws_sgm_path_kernel: one wave per path line, lane l holding j = 64 k + l for k < NJ.  Each step is a dependent
//     chain (the wave minimum of the previous pixel); the next pixel's candidate interval, costs and running sums are
//     loaded before the current pixel is worked.  The d +- 1 terms cross lanes by shuffles.  One launch per direction,
//     in order on one stream: the first writes S, the others add to it -- a pixel lies on one line per direction, so no
//     two waves of a launch touch the same sums.
//   * ws_sgm_wta_kernel: one wave per pixel: the minimum of (S, tie tag) over the candidates, the parabola on S, and
//     the fallbacks; lane 0 writes the float32 value.
//   * ws_unique_wta_kernel: that winner with the uniqueness test and the confidence of include/ws_stereo.h, on S or
//     (block route, no path kernel) on C itself.  Each lane keeps its best key and its runner-up's value, so the curve
//     is read once: the rival minimum m2 is a second wave minimum over what the lanes still hold.
//   * ws_pair_wta_kernel: the other view's map from the same volume ("both views from one volume").  One workgroup per
//     row and span of kPairSpan derived columns; a 64-bit LDS slot per derived column takes the minimum of the packed
//     keys (S, tie tag) that the base pixels' curves offer along the diagonal.
// Every store is a plain vector store.
#include "ws_sgm.h"
#include "ws_ct.h"

#include <type_traits>

namespace wsamd {

namespace {

constexpr int kSgmThreads = 256;
constexpr int kSgmTile = 64;                         // cost kernel: columns per workgroup (16 per wave)
constexpr int kSgmStrip = 32;                        // cost kernel: rows per workgroup
constexpr int kSgmMaxHalf = 31;                      // block_size <= 63
constexpr int kSgmCols = kSgmTile + 2 * kSgmMaxHalf; // column sums a tile needs at most
constexpr int kSgmColsPerWave = (kSgmCols + 3) / 4;
constexpr uint32_t kNoCandidate = 0xffffffffu;
constexpr int kUniqueBlocksPerCu = 8;                // uniqueness winner: 32 waves per CU, all resident
constexpr int kPairUnroll = 4;                       // diagonal winner: base columns a wave has in flight per trip
static_assert(kSgmThreads == 256 && kSgmTile == 64, "four waves, 16 output columns each");
static_assert(kSgmMaxNd <= 64 * 32 && kSgmMaxNd < 4096, "32 disparities per lane; 12-bit tie tags");

__device__ __forceinline__ uint32_t pixel_cost(const uint8_t *l, const uint8_t *r, int ssd)
{
    const int a = (int)l[0] - (int)r[0], b = (int)l[1] - (int)r[1], c = (int)l[2] - (int)r[2];
    return ssd ? (uint32_t)(a * a + b * b + c * c) : (uint32_t)(abs(a) + abs(b) + abs(c));
}

__device__ __forceinline__ bool black(const uint8_t *p) { return (p[0] | p[1] | p[2]) == 0; }

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(kSgmThreads) void ws_sgm_kr_kernel(SgmArgs a)
{
    const long long n = (long long)a.w * a.h;
    const int rows = min(a.h1, a.h2), half = a.half;
    for (long long i = (long long)blockIdx.x * kSgmThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSgmThreads) {
        const int y = (int)(i / a.w), x = (int)(i % a.w);
        uint32_t kr = 0;
        if (!a.right) {
            if (y >= half && y < rows - half && x >= half && x < a.w1 - half && !black(a.L + (size_t)y * a.s1 + 3 * x)) {
                // d in [max(1, x - w2 + half + 1), min(maxD, x - half)], j = d - 1
                const int lo = max(0, x - a.w2 + half), hi = min(a.nd, x - half);
                kr = hi > lo ? (uint32_t)lo | (uint32_t)hi << 16 : kNoCandidate;
            }
        } else if (y < rows && !black(a.R + (size_t)y * a.s2 + 3 * x)) {
            const int left = min(x, half), right = min(a.w2 - x - 1, half), up = min(y, half), down = min(a.h2 - y - 1, half);
            // d in [minD, min(maxD, w1 - x - right)), j = d - minD
            const int hi = min(a.nd, a.w1 - x - right - a.d0);
            kr = (left + right) * (up + down) > 0 && hi > 0 ? (uint32_t)hi << 16 : kNoCandidate;
        }
        a.kr[i] = kr;
    }
}

// The window of output row y: image rows [lo, hi).  Left view: the full block; right view: the reference's clipped
// (up + down) rows.
__device__ __forceinline__ void window_rows(const SgmArgs &a, int rows, int y, int &lo, int &hi)
{
    if (!a.right) {
        lo = y - a.half;
        hi = y + a.half + 1;
    } else {
        lo = max(0, y - a.half);
        hi = min(min(a.h2 - 1, y + a.half), rows);
    }
}

// ... and of output column x: image columns [lo, hi) (of the left image, left view; of the right image, right view)
__device__ __forceinline__ void window_cols(const SgmArgs &a, int x, int &lo, int &hi)
{
    if (!a.right) {
        lo = x - a.half;
        hi = x + a.half + 1;
    } else {
        lo = max(0, x - a.half);
        hi = min(a.w2 - 1, x + a.half);
    }
}

template <typename CT>
__global__ __launch_bounds__(kSgmThreads) void ws_sgm_cost_kernel(SgmArgs a)
{
    __shared__ uint32_t col[kSgmCols][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (a.w + kSgmTile - 1) / kSgmTile, njc = (a.nd + 63) / 64;
    int b = blockIdx.x;
    const int tx = b % ntx;
    b /= ntx;
    const int jc = b % njc, sy = b / njc;
    const int x0 = tx * kSgmTile, j = jc * 64 + lane, d = a.d0 + j;
    const int y0 = sy * kSgmStrip, y1 = min(a.h, y0 + kSgmStrip);
    const int half = a.half, ncol = kSgmTile + 2 * half, rows = min(a.h1, a.h2);
    const bool live = j < a.nd;
    CT *cost = static_cast<CT *>(a.cost);

    uint32_t cs[kSgmColsPerWave]; // column c = wave + 4 i of the tile: image column x0 - half + c
#pragma unroll
    for (int i = 0; i < kSgmColsPerWave; ++i) cs[i] = 0;
    // add (sign 1) or remove (sign -1) image row yy from the column sums (mod 2^32: the sums that count are exact)
    const auto row = [&](int yy, uint32_t sign) {
        if (yy < 0 || yy >= rows) return;
        const uint8_t *lrow = a.L + (size_t)yy * a.s1, *rrow = a.R + (size_t)yy * a.s2;
#pragma unroll
        for (int i = 0; i < kSgmColsPerWave; ++i) {
            const int c = wave + 4 * i;
            const int xi = x0 - half + c;
            const int xl = a.right ? xi + d : xi, xr = a.right ? xi : xi - d;
            uint32_t v = 0;
            if (c < ncol && live && xl >= 0 && xl < a.w1 && xr >= 0 && xr < a.w2) v = pixel_cost(lrow + 3 * xl, rrow + 3 * xr, a.ssd);
            cs[i] += sign * v;
        }
    };
    int ra, rb;
    window_rows(a, rows, y0, ra, rb);
    rb = ra;
    for (int y = y0; y < y1; ++y) {
        int na, nb;
        window_rows(a, rows, y, na, nb);
        for (; rb < nb; ++rb) row(rb, 1u);
        for (; ra < na; ++ra) row(ra, 0xffffffffu);
#pragma unroll
        for (int i = 0; i < kSgmColsPerWave; ++i)
            if (wave + 4 * i < ncol) col[wave + 4 * i][lane] = cs[i];
        __syncthreads();
        uint32_t acc = 0;
        int ca = 0, cb = 0;
        for (int t = 0; t < kSgmTile / 4; ++t) {
            const int x = x0 + wave * (kSgmTile / 4) + t;
            if (x >= a.w) break;
            int xa, xb;
            window_cols(a, x, xa, xb);
            const int ka = xa - x0 + half, kb = xb - x0 + half; // in [0, ncol]
            if (t == 0) ca = cb = ka;
            for (; cb < kb; ++cb) acc += col[cb][lane];
            for (; ca < ka; ++ca) acc -= col[ca][lane];
            if (live) cost[((size_t)y * a.w + x) * a.nd + j] = (CT)acc;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool line_start(int dir, int line, int w, int h, int &x, int &y, int &dx, int &dy)
{
    switch (dir) {
    case 0: dx = 1; dy = 0; x = 0; y = line; return line < h;
    case 1: dx = -1; dy = 0; x = w - 1; y = line; return line < h;
    case 2: dx = 0; dy = 1; x = line; y = 0; return line < w;
    case 3: dx = 0; dy = -1; x = line; y = h - 1; return line < w;
    case 4: dx = 1; dy = 1; if (line < w) { x = line; y = 0; } else { x = 0; y = line - w + 1; } break;
    case 5: dx = -1; dy = -1; if (line < w) { x = line; y = h - 1; } else { x = w - 1; y = line - w; } break;
    case 6: dx = -1; dy = 1; if (line < w) { x = line; y = 0; } else { x = w - 1; y = line - w + 1; } break;
    default: dx = 1; dy = -1; if (line < w) { x = line; y = h - 1; } else { x = 0; y = line - w; } break;
    }
    return line < w + h - 1;
}

template <int NJ, typename CT, typename ST, bool FIRST>
__global__ __launch_bounds__(kSgmThreads) void ws_sgm_path_kernel(SgmArgs a, int dir)
{
    const int lane = threadIdx.x & 63;
    const int line = blockIdx.x * (kSgmThreads / 64) + (threadIdx.x >> 6);
    int x, y, dx, dy;
    if (!line_start(dir, line, a.w, a.h, x, y, dx, dy)) return; // (uniform over the wave)
    const CT *cost = static_cast<const CT *>(a.cost);
    ST *sum = static_cast<ST *>(a.sum);
    const int nd = a.nd;
    const uint32_t p1 = a.p1, p2 = a.p2, p21 = a.p2 - a.p1;

    uint32_t cc[NJ], nc[NJ], lq[NJ];
    ST sc[NJ], ns[NJ];
    const auto load = [&](size_t pix, uint32_t *c, ST *s) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int j = k * 64 + lane;
            c[k] = j < nd ? (uint32_t)cost[pix * nd + j] : 0u;
            if (!FIRST) s[k] = j < nd ? sum[pix * nd + j] : (ST)0;
        }
    };
    size_t pix = (size_t)y * a.w + x;
    uint32_t kr = a.kr[pix];
    load(pix, cc, sc);
    bool qnode = false;
    uint32_t mq = 0;
    int qlo = 0, qhi = 0;
#pragma unroll
    for (int k = 0; k < NJ; ++k) lq[k] = 0;
    for (;;) {
        const int nx = x + dx, ny = y + dy;
        const bool more = nx >= 0 && nx < a.w && ny >= 0 && ny < a.h;
        const size_t npix = more ? (size_t)ny * a.w + nx : pix;
        const uint32_t nkr = a.kr[npix];
        load(npix, nc, ns); // the next pixel's, while this one is worked
        const int lo = (int)(kr & 0xffff), hi = (int)(kr >> 16);
        if (hi > lo) {
            uint32_t m = 0xffffffffu, lr[NJ];
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const int j = k * 64 + lane;
                uint32_t best = 0;
                if (qnode) {
                    // Lr(q, j - 1) and Lr(q, j + 1): the neighbouring lane, across k at the wave's ends
                    uint32_t up = (uint32_t)__shfl_up((int)lq[k], 1);
                    const uint32_t up0 = k > 0 ? (uint32_t)__shfl((int)lq[k > 0 ? k - 1 : 0], 63) : 0u;
                    if (lane == 0) up = up0;
                    uint32_t dn = (uint32_t)__shfl_down((int)lq[k], 1);
                    const uint32_t dn0 = k + 1 < NJ ? (uint32_t)__shfl((int)lq[k + 1 < NJ ? k + 1 : k], 0) : 0u;
                    if (lane == 63) dn = dn0;
                    // min(Lr(q,j) - m, Lr(q,j-+1) - m + P1, P2), every term bounded by P2 before P1 is added
                    best = p2;
                    if (j >= qlo && j < qhi) best = min(best, lq[k] - mq);
                    if (j - 1 >= qlo && j - 1 < qhi) best = min(best, min(up - mq, p21) + p1);
                    if (j + 1 >= qlo && j + 1 < qhi) best = min(best, min(dn - mq, p21) + p1);
                }
                lr[k] = cc[k] + best; // < 2^30 + 2^31
                if (j >= lo && j < hi) {
                    m = min(m, lr[k]);
                    sum[pix * nd + j] = FIRST ? (ST)lr[k] : (ST)(sc[k] + (ST)lr[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < NJ; ++k) lq[k] = lr[k]; // (lq[k -+ 1] were read above: the previous pixel's)
            mq = wave_min(m);
            qlo = lo;
            qhi = hi;
            qnode = true;
        } else {
            qnode = false;
        }
        if (!more) break;
        x = nx;
        y = ny;
        pix = npix;
        kr = nkr;
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            cc[k] = nc[k];
            if (!FIRST) sc[k] = ns[k];
        }
    }
}

// ST: S as uint32_t / unsigned long long; the pair call's block route reads C (uint16_t / uint32_t) through it instead.
template <typename ST>
__global__ __launch_bounds__(kSgmThreads) void ws_sgm_wta_kernel(SgmArgs a, const ST *sum)
{
    const int lane = threadIdx.x & 63;
    const long long n = (long long)a.w * a.h;
    const long long waves = (long long)gridDim.x * (kSgmThreads / 64);
    for (long long i = (long long)blockIdx.x * (kSgmThreads / 64) + (threadIdx.x >> 6); i < n; i += waves) {
        const int y = (int)(i / a.w), x = (int)(i % a.w);
        const uint32_t kr = a.kr[i];
        float v = 0.0f;
        if (kr == kNoCandidate) {
            v = (float)(a.right ? -x : x);
        } else if (kr != 0) {
            const int lo = (int)(kr & 0xffff), hi = (int)(kr >> 16);
            const ST *s = sum + (size_t)i * a.nd;
            // (S, tag) with the tie rule in the tag: left view the largest j, right view the smallest
            unsigned long long key = ~0ull;
            for (int j = lo + lane; j < hi; j += 64) {
                const unsigned long long k = (unsigned long long)s[j] << 12 | (unsigned)(a.right ? j : 4095 - j);
                key = k < key ? k : key;
            }
            key = wave_min64(key);
            const int jb = a.right ? (int)(key & 4095) : 4095 - (int)(key & 4095);
            v = (float)(a.d0 + jb);
            if (a.subpixel && jb - 1 >= lo && jb + 1 < hi) {
                const long long sm = (long long)s[jb - 1], s0 = (long long)s[jb], sp = (long long)s[jb + 1];
                const long long num = sm - sp, den = sm - 2 * s0 + sp;
                if (den > 0) v = v + (float)((double)num / (2.0 * (double)den));
            }
        }
        if (lane == 0) a.out[(size_t)y * a.out_pitch + x] = v;
    }
}

// The winner with the rival minimum (uniqueness section of include/ws_stereo.h).  A lane visits j = lo + lane + 64 k, so
// jb - 1, jb, jb + 1 lie in three different lanes and a lane loses at most one entry to the exclusion: its best if
// that is one of the three, else an entry that is no smaller than its best.  Hence the lane's offer to m2 is its best,
// or its runner-up when its best is excluded.  VT: C as uint16_t / uint32_t, S as uint32_t / unsigned long long.
// The kernel is bound by the instructions a pixel takes, not by the bytes of its curve, so what is the same in every
// lane is kept scalar: the pixel index comes from the wave's number read as a uniform value, which makes the interval,
// the row / column split and the branches on the pixel's kind scalar work; the second minimum runs on 32-bit values
// where the stored type allows; and the confidence's division is done only when a plane was given.
template <typename VT>
__global__ __launch_bounds__(kSgmThreads) void ws_unique_wta_kernel(SgmArgs a, const VT *vol, UniqueArgs u)
{
    using MT = std::conditional_t<sizeof(VT) <= 4, uint32_t, unsigned long long>; // an offer to m2
    const int lane = threadIdx.x & 63;
    const uint32_t n = (uint32_t)a.w * (uint32_t)a.h; // (< 2^31: ws_validate_sgm)
    const uint32_t waves = gridDim.x * (kSgmThreads / 64);
    const uint32_t first = blockIdx.x * (kSgmThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long failed = 0, nodes = 0;
    for (uint32_t i = first; i < n; i += waves) {
        const uint32_t y = i / (uint32_t)a.w, x = i - y * (uint32_t)a.w;
        const uint32_t kr = a.kr[i];
        float v = 0.0f, conf = 0.0f;
        if (kr == kNoCandidate) {
            v = (float)(a.right ? -(int)x : (int)x);
        } else if (kr != 0) {
            const int lo = (int)(kr & 0xffff), hi = (int)(kr >> 16);
            const VT *s = vol + (size_t)i * a.nd;
            unsigned long long best = ~0ull; // the lane's best (value, tag) ...
            MT second = ~(MT)0;              // ... and its runner-up's value
            bool two = false;                // ... if it has one
            for (int j = lo + lane; j < hi; j += 64) {
                const unsigned long long val = (unsigned long long)s[j];
                const unsigned long long k = val << 12 | (unsigned)(a.right ? j : 4095 - j);
                const MT loser = k < best ? (MT)(best >> 12) : (MT)val;
                two = best != ~0ull;
                best = k < best ? k : best;
                second = loser < second ? loser : second;
            }
            const unsigned long long key = wave_min64(best);
            const int jb = a.right ? (int)(key & 4095) : 4095 - (int)(key & 4095);
            const unsigned long long smin = key >> 12;
            const int jl = a.right ? (int)(best & 4095) : 4095 - (int)(best & 4095);
            const bool mine = best != ~0ull && abs(jl - jb) >= 2; // the lane's best is a rival; else its runner-up is
            const bool contested = __ballot(mine || two) != 0;
            MT offer = mine ? (MT)(best >> 12) : second; // (a lane without a rival offers the largest value)
            if constexpr (sizeof(MT) == 4) offer = wave_min(offer);
            else offer = wave_min64(offer);
            const unsigned long long m2 = offer;
            v = (float)(a.d0 + jb);
            if (a.subpixel && jb - 1 >= lo && jb + 1 < hi) {
                const long long sm = (long long)s[jb - 1], s0 = (long long)s[jb], sp = (long long)s[jb + 1];
                const long long num = sm - sp, den = sm - 2 * s0 + sp;
                if (den > 0) v = v + (float)((double)num / (2.0 * (double)den));
            }
            conf = 1.0f;
            ++nodes;
            if (contested) {
                conf = 0.0f;
                if (u.conf && m2 > 0) conf = (float)((double)(m2 - smin) / (double)m2);
                if (m2 * (unsigned long long)(100 - u.ratio) < smin * 100ull) {
                    v = 0.0f;
                    ++failed;
                }
            }
        }
        if (lane == 0) {
            a.out[(size_t)y * a.out_pitch + x] = v;
            if (u.conf) u.conf[(size_t)y * u.conf_pitch + x] = conf;
        }
    }
    if (lane == 0 && nodes) { // (failed and nodes are uniform over the wave)
        if (failed) atomicAdd(u.counts, failed);
        atomicAdd(u.counts + 1, nodes);
    }
}

// The derived map of the pair call (include/ws_stereo.h, "both views from one volume").  The base view's pixel (y, x)
// offers vol(y, x, j) to the derived column c = x - d (base LEFT) or x + d (base RIGHT), d = d0 + j: the 64 entries a wave
// loads from one curve are contiguous and go to 64 different, consecutive slots.  Workgroup (y, span) owns the derived
// columns [c0, c0 + kPairSpan) of row y and visits the base columns that reach them, each for the part of its interval
// [lo, hi) that falls into the span, so every entry of the volume is read once over the grid.  A wave takes kPairUnroll
// neighbouring base columns per trip and issues their loads before the first LDS minimum.  The minimum over packed keys
// does not depend on the order of the offers; tag = j (base LEFT: the smallest d wins) or 4095 - j (base RIGHT: the
// largest).  Rows beyond the base map's, and columns nobody offers to, store 0.
template <typename VT>
__global__ __launch_bounds__(kSgmThreads) void ws_pair_wta_kernel(SgmArgs a, const VT *vol, float *out, int out_pitch, int wd, int hd)
{
    __shared__ unsigned long long slot[kPairSpan];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nspan = (wd + kPairSpan - 1) / kPairSpan;
    const int y = blockIdx.x / nspan, c0 = (blockIdx.x % nspan) * kPairSpan;
    const int cn = min(kPairSpan, wd - c0); // this span's columns
    for (int i = threadIdx.x; i < kPairSpan; i += kSgmThreads) slot[i] = ~0ull;
    __syncthreads();
    if (y < a.h && a.nd > 0) {
        const int sgn = a.right ? 1 : -1;
        // base columns that reach [c0, c0 + cn): x = c - sgn d for d in [d0, d0 + nd)
        const int xa = max(0, a.right ? c0 - a.d0 - a.nd + 1 : c0 + a.d0);
        const int xb = min(a.w, a.right ? c0 + cn - a.d0 : c0 + cn + a.d0 + a.nd - 1);
        const uint32_t *krow = a.kr + (size_t)y * a.w;
        const VT *vrow = vol + (size_t)y * a.w * a.nd;
        for (int x0 = xa + wave * kPairUnroll; x0 < xb; x0 += (kSgmThreads / 64) * kPairUnroll) {
            int jlo[kPairUnroll], jhi[kPairUnroll], more = 0;
#pragma unroll
            for (int u = 0; u < kPairUnroll; ++u) {
                const int x = x0 + u;
                jlo[u] = jhi[u] = 0;
                if (x >= xb) continue;
                const uint32_t kr = krow[x];
                if (kr == 0 || kr == kNoCandidate) continue;
                // c = x + sgn (d0 + j) in [c0, c0 + cn)
                const int ja = a.right ? c0 - x - a.d0 : x - a.d0 - c0 - cn + 1, jb = a.right ? c0 + cn - x - a.d0 : x - a.d0 - c0 + 1;
                jlo[u] = max((int)(kr & 0xffff), ja);
                jhi[u] = min((int)(kr >> 16), jb);
                more = max(more, jhi[u] - jlo[u]);
            }
            for (int k = 0; k < more; k += 64) {
                unsigned long long key[kPairUnroll];
#pragma unroll
                for (int u = 0; u < kPairUnroll; ++u) {
                    const int j = jlo[u] + k + lane;
                    key[u] = ~0ull;
                    if (j < jhi[u]) key[u] = (unsigned long long)vrow[(size_t)(x0 + u) * a.nd + j] << 12 | (unsigned)(a.right ? 4095 - j : j);
                }
#pragma unroll
                for (int u = 0; u < kPairUnroll; ++u) {
                    const int j = jlo[u] + k + lane;
                    const int c = x0 + u + sgn * (a.d0 + j) - c0;
                    if (j < jhi[u] && c >= 0 && c < cn) atomicMin(&slot[c], key[u]);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cn; i += kSgmThreads) {
        const unsigned long long key = slot[i];
        float v = 0.0f;
        if (key != ~0ull) {
            const int tag = (int)(key & 4095);
            v = (float)(a.d0 + (a.right ? 4095 - tag : tag)); // (d == 0, base RIGHT with minD 0: 0.0f, "no disparity")
        }
        out[(size_t)y * out_pitch + c0 + i] = v;
    }
}

template <int NJ, typename CT, typename ST>
hipError_t launch_paths(const SgmArgs &a, int paths, hipStream_t s)
{
    for (int dir = 0; dir < paths; ++dir) {
        const int lines = dir < 2 ? a.h : dir < 4 ? a.w : a.w + a.h - 1;
        const int blocks = (lines + kSgmThreads / 64 - 1) / (kSgmThreads / 64);
        if (dir == 0) ws_sgm_path_kernel<NJ, CT, ST, true><<<blocks, kSgmThreads, 0, s>>>(a, dir);
        else ws_sgm_path_kernel<NJ, CT, ST, false><<<blocks, kSgmThreads, 0, s>>>(a, dir);
    }
    return hipGetLastError();
}

template <typename CT, typename ST>
hipError_t launch_paths_nj(const SgmArgs &a, int paths, hipStream_t s)
{
    const int per_lane = (a.nd + 63) / 64;
    if (per_lane <= 1) return launch_paths<1, CT, ST>(a, paths, s);
    if (per_lane <= 2) return launch_paths<2, CT, ST>(a, paths, s);
    if (per_lane <= 4) return launch_paths<4, CT, ST>(a, paths, s);
    if (per_lane <= 8) return launch_paths<8, CT, ST>(a, paths, s);
    if (per_lane <= 16) return launch_paths<16, CT, ST>(a, paths, s);
    return launch_paths<32, CT, ST>(a, paths, s);
}

} // namespace

// The candidate intervals, the cost plane and, with paths > 0, the sums, on s.
static hipError_t launch_volumes(const SgmArgs &a, int paths, hipStream_t s)
{
    const long long n = (long long)a.w * a.h;
    const int grid = (int)std::min<long long>((n + kSgmThreads - 1) / kSgmThreads, 1 << 20);
    ws_sgm_kr_kernel<<<grid, kSgmThreads, 0, s>>>(a);
    if (a.nd > 0) {
        const long long blocks = (long long)((a.w + kSgmTile - 1) / kSgmTile) * ((a.nd + 63) / 64) * ((a.h + kSgmStrip - 1) / kSgmStrip);
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        if (a.TL) { // a census cost: the one implementation of its window sums, storing C in this layout
            CtMatchArgs c{};
            c.TL = a.TL; c.TR = a.TR; c.L = a.L; c.R = a.R;
            c.w1 = a.w1; c.h1 = a.h1; c.s1 = a.s1; c.w2 = a.w2; c.h2 = a.h2; c.s2 = a.s2;
            c.wide = a.census_wide; c.right = a.right; c.half = a.half; c.d0 = a.d0; c.nd = a.nd; c.w = a.w; c.h = a.h;
            c.cost = a.cost; c.cost16 = a.cost16;
            if (const hipError_t e = launch_census_match(c, true, s); e != hipSuccess) return e;
        } else if (a.cost16) ws_sgm_cost_kernel<uint16_t><<<(int)blocks, kSgmThreads, 0, s>>>(a);
        else ws_sgm_cost_kernel<uint32_t><<<(int)blocks, kSgmThreads, 0, s>>>(a);
        if (paths > 0) {
            hipError_t e;
            if (a.cost16 && !a.sum64) e = launch_paths_nj<uint16_t, uint32_t>(a, paths, s);
            else if (a.cost16) e = launch_paths_nj<uint16_t, unsigned long long>(a, paths, s);
            else if (!a.sum64) e = launch_paths_nj<uint32_t, uint32_t>(a, paths, s);
            else e = launch_paths_nj<uint32_t, unsigned long long>(a, paths, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

hipError_t launch_sgm(const SgmArgs &a, int paths, hipStream_t s)
{
    if (const hipError_t e = launch_volumes(a, paths, s); e != hipSuccess) return e;
    const long long n = (long long)a.w * a.h;
    const int wgrid = (int)std::min<long long>((n + 3) / 4, 1 << 20);
    if (paths > 0) {
        if (a.sum64) ws_sgm_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const unsigned long long *>(a.sum));
        else ws_sgm_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.sum));
    } else {
        if (a.cost16) ws_sgm_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint16_t *>(a.cost));
        else ws_sgm_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.cost));
    }
    return hipGetLastError();
}

hipError_t launch_unique(const SgmArgs &a, const UniqueArgs &u, int paths, hipStream_t s)
{
    if (const hipError_t e = launch_volumes(a, paths, s); e != hipSuccess) return e;
    // a grid the device holds at once: each wave walks its share of the pixels and adds to the counts once at its end
    const long long n = (long long)a.w * a.h;
    const int wgrid = (int)std::min<long long>((n + 3) / 4, (long long)kUniqueBlocksPerCu * std::max(1, u.num_cus));
    if (paths > 0) {
        if (a.sum64) ws_unique_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const unsigned long long *>(a.sum), u);
        else ws_unique_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.sum), u);
    } else {
        if (a.cost16) ws_unique_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint16_t *>(a.cost), u);
        else ws_unique_wta_kernel<<<wgrid, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.cost), u);
    }
    return hipGetLastError();
}

hipError_t launch_pair_wta(const SgmArgs &a, int paths, float *out, int out_pitch, int wd, int hd, hipStream_t s)
{
    const long long blocks = (long long)hd * ((wd + kPairSpan - 1) / kPairSpan);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (paths > 0) {
        if (a.sum64) ws_pair_wta_kernel<<<(int)blocks, kSgmThreads, 0, s>>>(a, static_cast<const unsigned long long *>(a.sum), out, out_pitch, wd, hd);
        else ws_pair_wta_kernel<<<(int)blocks, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.sum), out, out_pitch, wd, hd);
    } else {
        if (a.cost16) ws_pair_wta_kernel<<<(int)blocks, kSgmThreads, 0, s>>>(a, static_cast<const uint16_t *>(a.cost), out, out_pitch, wd, hd);
        else ws_pair_wta_kernel<<<(int)blocks, kSgmThreads, 0, s>>>(a, static_cast<const uint32_t *>(a.cost), out, out_pitch, wd, hd);
    }
    return hipGetLastError();
}

} // namespace wsamd
