// ws_rectify.hip -- the forward warp of image rectification:
//   warpPerspective(leftImage_, leftRectifiedImage_, H_, size)     rectification.cpp:486-489
//   warpPerspective(rightImage_, rightRectifiedImage_, Hp_, size)   rectification.cpp:490-493
// INTER_LINEAR, BORDER_CONSTANT 0, CV_8UC3 in and out (warpPerspective creates dst with the source's type).
//
// OpenCV is not vendored by the reference: this restates OpenCV 4.x's fixed-point INTER_LINEAR path (the one
// OpenCV <= 4.10 runs on x86: WarpPerspectiveInvoker + remapBilinear, INTER_BITS 5, INTER_REMAP_COEF_BITS 15).
// PARITY UNPINNED: later OpenCV releases may differ from it by one grey level.  Per destination pixel (x, y):
//   * column block: bw0 = min(1024 / min(16, dst_h), dst_w), xb = x - x mod bw0, x1 = x - xb
//     (for 16 rows or more this is the x & ~63 of the nearest warp in ws_consumers.hip);
//   * in double, left to right, no contraction (-ffp-contract=off), correctly rounded division:
//     X0 = M0*xb + M1*y + M2 (Y0, W0 likewise), W = W0 + M6*x1, W = W != 0 ? 32/W : 0,
//     fX = clamp((X0 + M0*x1)*W, INT_MIN, INT_MAX), X = rint(fX) (half to even); Y likewise;
//   * taps sx = sat16(X >> 5), sy = sat16(Y >> 5), fractions ax = X & 31, ay = Y & 31, weights
//     (32-ax)(32-ay)*32, ax(32-ay)*32, (32-ax)ay*32, ax*ay*32 (exact, sum 32768);
//   * per channel (sum w*tap + 16384) >> 15, a tap outside the source reading 0.
// Shape: four consecutive destination pixels per thread (one dword-aligned 12-byte store when the row allows it),
// the two taps of a source row read as dwords and cut out with v_alignbyte.  A gather plus a short FP64 chain.
#include "ws_device.h"
#include "ws_rectify.h"

namespace wsamd {

constexpr int kRectPx = 4;       // destination pixels per thread
constexpr int kRectThreads = 256;

struct RectifyArgs {
    const uint8_t *src;
    size_t span;  // bytes of the source the kernel may read: sp*(sh-1) + 3*sw
    int sw, sh, sp;
    uint8_t *dst;
    int dw, dh, dp;
    int bw0;      // OpenCV's column block width
    double m[9];  // destination -> source
};

__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// The 6 bytes [off, off + 6) of the source -- both taps of one source row -- as bytes 0..3 in lo, 4..5 in hi.
// Dword loads from the aligned address below, as long as every dword lies inside the source's span; else bytes.
__device__ __forceinline__ void row_taps(const RectifyArgs &g, size_t off, uint32_t &lo, uint32_t &hi)
{
    const uintptr_t base = reinterpret_cast<uintptr_t>(g.src);
    const uintptr_t p = base + off;
    const uintptr_t a = p & ~(uintptr_t)3;
    const uint32_t o = (uint32_t)(p & 3);
    const uintptr_t need = o == 3 ? 12 : 8; // bytes o..o+5 lie in 2 dwords, in 3 at o == 3
    if (a >= base && a + need <= base + g.span) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(a);
        const uint32_t d0 = q[0], d1 = q[1];
        const uint32_t d2 = o == 3 ? q[2] : 0u;
        lo = __builtin_amdgcn_alignbyte(d1, d0, o);
        hi = __builtin_amdgcn_alignbyte(d2, d1, o);
    } else {
        const uint8_t *b = g.src + off;
        lo = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        hi = (uint32_t)b[4] | ((uint32_t)b[5] << 8);
    }
}

__device__ __forceinline__ uint32_t byte_of(uint32_t v, int k) { return (v >> (8 * k)) & 0xffu; }

// one tap of the border path: 0 outside the source
__device__ __forceinline__ uint32_t tap(const RectifyArgs &g, int tx, int ty, int c)
{
    if ((unsigned)tx >= (unsigned)g.sw || (unsigned)ty >= (unsigned)g.sh) return 0u;
    return g.src[(size_t)ty * g.sp + 3 * (size_t)tx + c];
}

__global__ void __launch_bounds__(kRectThreads) ws_rectify_kernel(const RectifyArgs g)
{
    const int x0 = (blockIdx.x * kRectThreads + threadIdx.x) * kRectPx;
    const int y = blockIdx.y;
    if (x0 >= g.dw) return;
    uint32_t packed[3] = {0u, 0u, 0u}; // the 12 output bytes of the thread's 4 pixels
    int x1 = x0 % g.bw0, xb = x0 - x1;  // (one division per thread; the next pixels step along the block)
    double X0 = g.m[0] * xb + g.m[1] * y + g.m[2];
    double Y0 = g.m[3] * xb + g.m[4] * y + g.m[5];
    double W0 = g.m[6] * xb + g.m[7] * y + g.m[8];
#pragma unroll
    for (int i = 0; i < kRectPx; ++i) {
        if (i > 0 && ++x1 == g.bw0) { // the next column block: its base row terms, as OpenCV recomputes them
            xb += g.bw0;
            x1 = 0;
            X0 = g.m[0] * xb + g.m[1] * y + g.m[2];
            Y0 = g.m[3] * xb + g.m[4] * y + g.m[5];
            W0 = g.m[6] * xb + g.m[7] * y + g.m[8];
        }
        double W = W0 + g.m[6] * x1;
        W = W != 0.0 ? 32.0 / W : 0.0;
        const double fX = fmax((double)INT_MIN, fmin((double)INT_MAX, (X0 + g.m[0] * x1) * W));
        const double fY = fmax((double)INT_MIN, fmin((double)INT_MAX, (Y0 + g.m[3] * x1) * W));
        const int X = (int)rint(fX), Y = (int)rint(fY); // round half to even, like cvRound
        const int sx = sat16(X >> 5), sy = sat16(Y >> 5);
        const int ax = X & 31, ay = Y & 31;
        const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32;
        const int w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
        uint32_t px = 0u; // the pixel's three bytes
        if (sx >= 0 && sx < g.sw - 1 && sy >= 0 && sy < g.sh - 1) {
            uint32_t l0, h0, l1, h1;
            const size_t off = (size_t)sy * g.sp + 3 * (size_t)sx;
            row_taps(g, off, l0, h0);
            row_taps(g, off + g.sp, l1, h1);
            const uint32_t r0b = (l0 >> 24) | (h0 << 8), r1b = (l1 >> 24) | (h1 << 8); // the right taps' 3 bytes
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = w00 * (int)byte_of(l0, c) + w01 * (int)byte_of(r0b, c) + w10 * (int)byte_of(l1, c) +
                              w11 * (int)byte_of(r1b, c) + 16384;
                px |= (uint32_t)(v >> 15) << (8 * c);
            }
        } else if (sx < g.sw && sx + 1 >= 0 && sy < g.sh && sy + 1 >= 0) { // part of the footprint inside
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = w00 * (int)tap(g, sx, sy, c) + w01 * (int)tap(g, sx + 1, sy, c) +
                              w10 * (int)tap(g, sx, sy + 1, c) + w11 * (int)tap(g, sx + 1, sy + 1, c) + 16384;
                px |= (uint32_t)(v >> 15) << (8 * c);
            }
        }
        // bytes 3i .. 3i+2 of the 12
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            packed[k >> 2] |= byte_of(px, c) << (8 * (k & 3));
        }
    }
    uint8_t *row = g.dst + (size_t)y * g.dp + 3 * (size_t)x0;
    if (x0 + kRectPx <= g.dw && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(row);
        q[0] = packed[0];
        q[1] = packed[1];
        q[2] = packed[2];
    } else {
        const int n = 3 * min(kRectPx, g.dw - x0);
        for (int k = 0; k < n; ++k) row[k] = (uint8_t)byte_of(packed[k >> 2], k & 3);
    }
}

hipError_t launch_rectify(const uint8_t *src, int sw, int sh, int sp, const double minv[9], uint8_t *dst, int dw, int dh,
                          int dp, hipStream_t s)
{
    RectifyArgs g{};
    g.src = src;
    g.sw = sw; g.sh = sh; g.sp = sp;
    g.span = (size_t)sp * (sh - 1) + 3 * (size_t)sw;
    g.dst = dst;
    g.dw = dw; g.dh = dh; g.dp = dp;
    g.bw0 = std::min(1024 / std::min(16, dh), dw);
    for (int i = 0; i < 9; ++i) g.m[i] = minv[i];
    hipLaunchKernelGGL(ws_rectify_kernel, dim3(ceil_div(dw, kRectThreads * kRectPx), dh), dim3(kRectThreads), 0, s, g);
    return hipGetLastError();
}

} // namespace wsamd
