// ws_ct.hip -- the census-transform matching cost (extension; the rules are in include/ws_stereo.h).  Integer work only.
//   * ws_census_transform_kernel: one workgroup per tile of 32 x 8 pixels.  The tile's grey values and the rx / ry halo
//     are computed once from the BGR bytes into LDS (255 outside the image: never below a centre); each lane builds its
//     descriptor from LDS.  Once per image, never per hypothesis.
//   * ws_census_match_kernel: the window sums of popcount(T_L xor T_R) of 64 columns x kCtStrip rows per workgroup, over
//     the whole disparity range in chunks of 64 lanes: lane = disparity, as ws_sgm_cost_kernel.  Each lane keeps the
//     column sums of its disparity for a quarter of the tile's columns (plus the window's halo) in registers and slides
//     them down the strip; the sums go through LDS (16 bits: a column holds at most 62 * 63); each wave then slides the
//     window along 16 columns.  Two sinks:
//       (a) winner-take-all: per pixel the wave minimum of (C << 6 | tie tag) over the chunk's candidates, merged by lane
//           0 into the pixel's running best in LDS with the view's tie rule; a chunk owns 62 candidates, lanes 0 and 63
//           hold their neighbours' costs so that the parabola never crosses a chunk seam.  After the last chunk every
//           thread finishes pixels: fallbacks, zeros outside the region, the parabola, the float32 store.  The cost
//           volume never touches memory.
//       (b) C(p, j) in semi-global matching's layout and width (ws_sgm.hip reads it).
// Every store is a plain vector store.
#include "ws_ct.h"

namespace wsamd {

namespace {

constexpr int kCtTw = 32, kCtTh = 8; // transform tile
constexpr int kCtColsPerWave = (kCtCols + 3) / 4;
constexpr uint32_t kNone = 0xffffffffu;
static_assert(kCtThreads == 256 && kCtTile == 64 && kCtTw * kCtTh == kCtThreads, "four waves, 16 output columns each");
static_assert(62 * 63 < 65536 && 62 * 63 * 63 < (1 << 26), "column sums in 16 bits; C << 6 in 32");

template <int RX, int RY, typename OT>
__global__ __launch_bounds__(kCtThreads) void ws_census_transform_kernel(const uint8_t *img, int w, int h, int stride, OT *out, int pitch)
{
    constexpr int GW = kCtTw + 2 * RX, GH = kCtTh + 2 * RY;
    __shared__ uint8_t g[GH][GW];
    const int ntx = (w + kCtTw - 1) / kCtTw;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    for (int i = threadIdx.x; i < GW * GH; i += kCtThreads) {
        const int gy = i / GW, gx = i % GW;
        const int y = ty * kCtTh - RY + gy, x = tx * kCtTw - RX + gx;
        uint32_t v = 255;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const uint8_t *p = img + (size_t)y * stride + 3 * x;
            v = (1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14;
        }
        g[gy][gx] = (uint8_t)v;
    }
    __syncthreads();
    const int lx = threadIdx.x % kCtTw, ly = threadIdx.x / kCtTw;
    const int x = tx * kCtTw + lx, y = ty * kCtTh + ly;
    if (x >= w || y >= h) return;
    const uint32_t c = g[ly + RY][lx + RX];
    uint32_t lo = 0, hi = 0;
    int k = 0;
#pragma unroll
    for (int dy = -RY; dy <= RY; ++dy)
#pragma unroll
        for (int dx = -RX; dx <= RX; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const uint32_t bit = g[ly + RY + dy][lx + RX + dx] < c ? 1u : 0u;
            if (k < 32) lo |= bit << (k & 31);
            else hi |= bit << (k & 31);
            ++k;
        }
    out[(size_t)y * pitch + x] = (OT)((unsigned long long)hi << 32 | lo);
}

__device__ __forceinline__ uint32_t hamming(uint32_t a, uint32_t b) { return (uint32_t)__builtin_popcount(a ^ b); }
__device__ __forceinline__ uint32_t hamming(unsigned long long a, unsigned long long b)
{
    const unsigned long long x = a ^ b;
    return (uint32_t)__builtin_popcount((uint32_t)x) + (uint32_t)__builtin_popcount((uint32_t)(x >> 32));
}

__device__ __forceinline__ bool black(const uint8_t *p) { return (p[0] | p[1] | p[2]) == 0; }

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// The window of output row y: image rows [lo, hi).  Left view: the full block; right view: the reference's clipped
// (up + down) rows.
__device__ __forceinline__ void window_rows(const CtMatchArgs &a, int rows, int y, int &lo, int &hi)
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
__device__ __forceinline__ void window_cols(const CtMatchArgs &a, int x, int &lo, int &hi)
{
    if (!a.right) {
        lo = x - a.half;
        hi = x + a.half + 1;
    } else {
        lo = max(0, x - a.half);
        hi = min(a.w2 - 1, x + a.half);
    }
}

// The candidate indices [lo, hi) of pixel (y, x) from the geometry alone (the region and the black test come later).
__device__ __forceinline__ void candidates(const CtMatchArgs &a, int y, int x, int &lo, int &hi)
{
    if (!a.right) {
        // d in [max(1, x - w2 + half + 1), min(maxD, x - half)], j = d - 1
        lo = max(0, x - a.w2 + a.half);
        hi = min(a.nd, x - a.half);
    } else {
        const int left = min(x, a.half), right = min(a.w2 - x - 1, a.half), up = min(y, a.half), down = min(a.h2 - y - 1, a.half);
        // d in [minD, min(maxD, w1 - x - right)), j = d - minD
        lo = 0;
        hi = (left + right) * (up + down) > 0 ? min(a.nd, a.w1 - x - right - a.d0) : 0;
    }
}

template <typename DT, typename CT, bool VOLUME>
__global__ __launch_bounds__(kCtThreads) void ws_census_match_kernel(CtMatchArgs a)
{
    constexpr int kPix = VOLUME ? 1 : kCtStrip * kCtTile;
    constexpr int kStep = VOLUME ? 64 : kCtWtaStep, kBase = VOLUME ? 0 : -1;
    __shared__ uint16_t col[kCtCols][64];
    __shared__ uint32_t best_j[kPix], best_c[kPix], best_m[kPix], best_p[kPix]; // the winner, its cost, C(j - 1), C(j + 1)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (a.w + kCtTile - 1) / kCtTile;
    const int tx = blockIdx.x % ntx, sy = blockIdx.x / ntx;
    const int x0 = tx * kCtTile;
    const int y0 = sy * kCtStrip, y1 = min(a.h, y0 + kCtStrip);
    const int half = a.half, ncol = kCtTile + 2 * half, rows = min(a.h1, a.h2);
    const DT *TL = static_cast<const DT *>(a.TL), *TR = static_cast<const DT *>(a.TR);
    CT *cost = static_cast<CT *>(a.cost);

    if (!VOLUME) {
        for (int i = threadIdx.x; i < kPix; i += kCtThreads) best_j[i] = kNone;
        __syncthreads();
    }
    const int nchunks = (a.nd + kStep - 1) / kStep;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int j = ch * kStep + kBase + lane, d = a.d0 + j;
        const bool live = j >= 0 && j < a.nd;
        uint32_t cs[kCtColsPerWave]; // column c = wave + 4 i of the tile: image column x0 - half + c
#pragma unroll
        for (int i = 0; i < kCtColsPerWave; ++i) cs[i] = 0;
        // add (sign 1) or remove (sign -1) image row yy from the column sums (mod 2^32: the sums that count are exact)
        const auto row = [&](int yy, uint32_t sign) {
            if (yy < 0 || yy >= rows) return;
            const DT *lrow = TL + (size_t)yy * a.w1, *rrow = TR + (size_t)yy * a.w2;
#pragma unroll
            for (int i = 0; i < kCtColsPerWave; ++i) {
                const int c = wave + 4 * i;
                const int xi = x0 - half + c;
                const int xl = a.right ? xi + d : xi, xr = a.right ? xi : xi - d;
                uint32_t v = 0;
                if (c < ncol && live && xl >= 0 && xl < a.w1 && xr >= 0 && xr < a.w2) v = hamming(lrow[xl], rrow[xr]);
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
            for (int i = 0; i < kCtColsPerWave; ++i)
                if (wave + 4 * i < ncol) col[wave + 4 * i][lane] = (uint16_t)cs[i];
            __syncthreads();
            uint32_t acc = 0;
            int ca = 0, cb = 0;
            for (int t = 0; t < kCtTile / 4; ++t) {
                const int x = x0 + wave * (kCtTile / 4) + t;
                if (x >= a.w) break;
                int xa, xb;
                window_cols(a, x, xa, xb);
                const int ka = xa - x0 + half, kb = xb - x0 + half; // in [0, ncol]
                if (t == 0) ca = cb = ka;
                for (; cb < kb; ++cb) acc += col[cb][lane];
                for (; ca < ka; ++ca) acc -= col[ca][lane];
                if (VOLUME) {
                    if (live) cost[((size_t)y * a.w + x) * a.nd + j] = (CT)acc;
                } else {
                    int lo, hi;
                    candidates(a, y, x, lo, hi);
                    // (C, tag) with the tie rule in the tag: left view the largest j, right view the smallest
                    const bool mine = lane >= 1 && lane <= kCtWtaStep && j >= lo && j < hi;
                    const uint32_t key = wave_min(mine ? acc << 6 | (uint32_t)(a.right ? lane : 63 - lane) : kNone);
                    if (key != kNone) { // (uniform over the wave)
                        const int lb = a.right ? (int)(key & 63) : 63 - (int)(key & 63);
                        const uint32_t cm = (uint32_t)__shfl((int)acc, lb - 1), cp = (uint32_t)__shfl((int)acc, lb + 1);
                        if (lane == 0) {
                            const int pi = (y - y0) * kCtTile + (x - x0);
                            const uint32_t c = key >> 6;
                            // chunks come in rising j: the left view keeps the later of two equal costs
                            if (best_j[pi] == kNone || (a.right ? c < best_c[pi] : c <= best_c[pi])) {
                                best_j[pi] = (uint32_t)(ch * kStep + kBase + lb);
                                best_c[pi] = c;
                                best_m[pi] = cm;
                                best_p[pi] = cp;
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (VOLUME) return;
    __syncthreads();
    for (int pi = threadIdx.x; pi < kPix; pi += kCtThreads) {
        const int y = y0 + pi / kCtTile, x = x0 + pi % kCtTile;
        if (y >= y1 || x >= a.w) continue;
        float v = 0.0f;
        const bool inside = a.right ? y < rows && !black(a.R + (size_t)y * a.s2 + 3 * x)
                                    : y >= half && y < rows - half && x >= half && x < a.w1 - half && !black(a.L + (size_t)y * a.s1 + 3 * x);
        if (inside) {
            int lo, hi;
            candidates(a, y, x, lo, hi);
            if (hi > lo) {
                const int jb = (int)best_j[pi];
                v = (float)(a.d0 + jb);
                if (a.subpixel && jb - 1 >= lo && jb + 1 < hi) {
                    const long long sm = (long long)best_m[pi], s0 = (long long)best_c[pi], sp = (long long)best_p[pi];
                    const long long num = sm - sp, den = sm - 2 * s0 + sp;
                    if (den > 0) v = v + (float)((double)num / (2.0 * (double)den));
                }
            } else {
                v = (float)(a.right ? -x : x);
            }
        }
        a.out[(size_t)y * a.out_pitch + x] = v;
    }
}

} // namespace

hipError_t launch_census_transform(const uint8_t *img, int w, int h, int stride, int cost, void *out, int out_pitch, bool widen,
                                   hipStream_t s)
{
    const long long blocks = (long long)((w + kCtTw - 1) / kCtTw) * ((h + kCtTh - 1) / kCtTh);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    auto *o64 = static_cast<unsigned long long *>(out);
    if (cost == WS_COST_CENSUS_9X7) ws_census_transform_kernel<4, 3, unsigned long long><<<(int)blocks, kCtThreads, 0, s>>>(img, w, h, stride, o64, out_pitch);
    else if (widen) ws_census_transform_kernel<2, 2, unsigned long long><<<(int)blocks, kCtThreads, 0, s>>>(img, w, h, stride, o64, out_pitch);
    else ws_census_transform_kernel<2, 2, uint32_t><<<(int)blocks, kCtThreads, 0, s>>>(img, w, h, stride, static_cast<uint32_t *>(out), out_pitch);
    return hipGetLastError();
}

hipError_t launch_census_match(const CtMatchArgs &a, bool volume, hipStream_t s)
{
    const long long blocks = census_match_workgroups(a.w, a.h);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (volume && a.nd <= 0) return hipSuccess;
    const int g = (int)blocks;
    if (!volume) {
        if (a.wide) ws_census_match_kernel<unsigned long long, uint32_t, false><<<g, kCtThreads, 0, s>>>(a);
        else ws_census_match_kernel<uint32_t, uint32_t, false><<<g, kCtThreads, 0, s>>>(a);
    } else if (a.cost16) {
        if (a.wide) ws_census_match_kernel<unsigned long long, uint16_t, true><<<g, kCtThreads, 0, s>>>(a);
        else ws_census_match_kernel<uint32_t, uint16_t, true><<<g, kCtThreads, 0, s>>>(a);
    } else {
        if (a.wide) ws_census_match_kernel<unsigned long long, uint32_t, true><<<g, kCtThreads, 0, s>>>(a);
        else ws_census_match_kernel<uint32_t, uint32_t, true><<<g, kCtThreads, 0, s>>>(a);
    }
    return hipGetLastError();
}

} // namespace wsamd
