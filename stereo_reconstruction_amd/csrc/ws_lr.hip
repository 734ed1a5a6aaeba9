// ws_lr.hip -- the left-right consistency check and its occlusion fill (extension; the rules are in include/ws_stereo.h).
// Both are O(w h) passes over two float32 maps, bound by memory, with no MFMA:
//   * ws_lr_check_kernel: one workgroup per map row, one pixel per lane per step along the row.  The partner value is a
//     gather from the same row of the other map, within the row's disparity range of the pixel: mostly L1/L2 hits.  Each
//     lane writes its output value and a state byte; a wave counts its failures with a ballot and a popcount per step and
//     adds them with one 64-bit global atomic at the end.  The atomics go to kLrSlots counters per map, 128 bytes apart:
//     every wave of a 4K map on ONE address serialised them (1.9 ms measured, profiles/lr/); ws_lr_count_kernel sums them.
//   * ws_lr_fill_kernel: one workgroup per map row.  The nearest passed column at or left of x is an inclusive max-scan
//     of (passed ? x : -1), the nearest at or right of x an inclusive min-scan of (passed ? x : INT_MAX) from the right.
//     Each lane scans 4 columns, the 64 lanes of a wave scan with shuffles, the 4 waves are joined through LDS, and a row
//     wider than one chunk (1024 columns) carries the scan from chunk to chunk.  The right-to-left pass stores the right
//     source's value into the failed pixels; the left-to-right pass combines it with the left source's (fminf).
// Every store is a plain vector store.
#include "ws_device.h"
#include "ws_kernels.h"

#include <limits.h>

namespace wsamd {

constexpr int kLrThreads = 256;
constexpr int kLrPer = 4;                          // fill: columns per lane
constexpr int kLrChunk = kLrThreads * kLrPer;      // fill: columns per workgroup pass
constexpr int kLrWaves = kLrThreads / 64;
static_assert(kLrSlots == 64, "ws_lr_count_kernel: one lane per counter slot");

// blockIdx.x: a row of map 0 (< h[0]) or of map 1
__global__ __launch_bounds__(kLrThreads) void ws_lr_check_kernel(LrMaps m, float max_diff, unsigned long long *slots)
{
    const int row = blockIdx.x;
    const int k = row < m.h[0] ? 0 : 1; // (uniform over the workgroup)
    const int y = k ? row - m.h[0] : row;
    const int o = 1 - k;
    const int w = m.w[k], wb = m.w[o];
    const bool partner_row = y < m.h[o];
    const double s = k ? 1.0 : -1.0;
    const float *a = m.in[k] + (size_t)y * m.in_pitch[k];
    const float *b = m.in[o] + (size_t)(partner_row ? y : 0) * m.in_pitch[o];
    float *out = m.out[k] + (size_t)y * m.out_pitch[k];
    uint8_t *st = m.state[k] ? m.state[k] + (size_t)y * lr_state_pitch(w) : nullptr;
    unsigned long long failures = 0; // this wave's (the same in every lane)
    for (int x0 = 0; x0 < w; x0 += kLrThreads) {
        const int x = x0 + (int)threadIdx.x;
        bool failed = false;
        if (x < w) {
            const float v = a[x];
            uint8_t state = kLrEmpty;
            if (v != 0.0f) {
                bool pass = false;
                if (__builtin_isfinite(v) && partner_row) {
                    // in double: exact for |rint(v)| < 2^53, and anything larger lies far outside [0, wb)
                    const double p = (double)x + s * (double)rintf(v);
                    if (p >= 0.0 && p < (double)wb) pass = fabsf(v - b[(long long)p]) <= max_diff;
                }
                state = pass ? kLrPassed : kLrFailed;
                failed = !pass;
            }
            out[x] = state == kLrPassed ? v : 0.0f;
            if (st) st[x] = state;
        }
        failures += (unsigned long long)__popcll(__ballot(failed));
    }
    if ((threadIdx.x & 63) == 0 && failures) atomicAdd(&slots[(k * kLrSlots + row % kLrSlots) * kLrSlotWords], failures);
}

// counts[k] = the sum of map k's kLrSlots counters: one wave per map
__global__ __launch_bounds__(128) void ws_lr_count_kernel(const unsigned long long *slots, unsigned long long *counts)
{
    unsigned long long v = slots[threadIdx.x * kLrSlotWords];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) counts[threadIdx.x >> 6] = v;
}

__global__ __launch_bounds__(kLrThreads) void ws_lr_fill_kernel(LrMaps m)
{
    __shared__ int tot[2][kLrWaves]; // per-wave scan totals, alternating between consecutive chunks
    const int row = blockIdx.x;
    const int k = row < m.h[0] ? 0 : 1;
    const int y = k ? row - m.h[0] : row;
    const int w = m.w[k];
    const uint8_t *st = m.state[k] + (size_t)y * lr_state_pitch(w);
    float *out = m.out[k] + (size_t)y * m.out_pitch[k];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunks = (w + kLrChunk - 1) / kLrChunk;
    // the 4 states of this lane's columns (the state row is padded to a multiple of 4 bytes: a dword never leaves it)
    auto states = [&](int base) -> uint32_t { return base < w ? *reinterpret_cast<const uint32_t *>(st + base) : 0u; };
    auto is = [&](uint32_t word, int base, int j, uint8_t what) { return base + j < w && ((word >> (8 * j)) & 0xff) == what; };
    int it = 0;

    // right to left: r = the nearest passed column >= x; a failed pixel takes its value (0 if there is none)
    int carry = INT_MAX;
    for (int c = chunks - 1; c >= 0; --c, ++it) {
        const int base = c * kLrChunk + t * kLrPer;
        const uint32_t word = states(base);
        int r[kLrPer], acc = INT_MAX;
        for (int j = kLrPer - 1; j >= 0; --j) {
            if (is(word, base, j, kLrPassed)) acc = base + j;
            r[j] = acc;
        }
        int sfx = acc; // inclusive suffix-min over the lanes >= this one
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_down(sfx, off);
            if (lane + off < 64) sfx = min(sfx, v);
        }
        if (lane == 0) tot[it & 1][wave] = sfx;
        __syncthreads();
        int after = __shfl_down(sfx, 1);
        if (lane == 63) after = INT_MAX;
        int next = carry;
        for (int v = 0; v < kLrWaves; ++v) {
            if (v > wave) after = min(after, tot[it & 1][v]);
            next = min(next, tot[it & 1][v]);
        }
        after = min(after, carry);
        for (int j = 0; j < kLrPer; ++j)
            if (is(word, base, j, kLrFailed)) {
                const int ri = min(r[j], after);
                if (ri != INT_MAX) out[base + j] = out[ri];
            }
        carry = next;
    }
    // left to right: l = the nearest passed column <= x; fminf with what the first pass left (a passed value is never 0)
    carry = -1;
    for (int c = 0; c < chunks; ++c, ++it) {
        const int base = c * kLrChunk + t * kLrPer;
        const uint32_t word = states(base);
        int l[kLrPer], acc = -1;
        for (int j = 0; j < kLrPer; ++j) {
            if (is(word, base, j, kLrPassed)) acc = base + j;
            l[j] = acc;
        }
        int pre = acc; // inclusive prefix-max over the lanes <= this one
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(pre, off);
            if (lane >= off) pre = max(pre, v);
        }
        if (lane == 63) tot[it & 1][wave] = pre;
        __syncthreads();
        int before = __shfl_up(pre, 1);
        if (lane == 0) before = -1;
        int next = carry;
        for (int v = 0; v < kLrWaves; ++v) {
            if (v < wave) before = max(before, tot[it & 1][v]);
            next = max(next, tot[it & 1][v]);
        }
        before = max(before, carry);
        for (int j = 0; j < kLrPer; ++j)
            if (is(word, base, j, kLrFailed)) {
                const int li = max(l[j], before);
                if (li >= 0) {
                    const float vl = out[li], vr = out[base + j]; // (this lane stored vr in the first pass)
                    out[base + j] = vr != 0.0f ? fminf(vl, vr) : vl;
                }
            }
        carry = next;
    }
}

hipError_t launch_lr_check(const LrMaps &m, float max_diff, unsigned long long *slots, unsigned long long *counts, hipStream_t s)
{
    hipLaunchKernelGGL(ws_lr_check_kernel, dim3((unsigned)(m.h[0] + m.h[1])), dim3(kLrThreads), 0, s, m, max_diff, slots);
    hipLaunchKernelGGL(ws_lr_count_kernel, dim3(1), dim3(2 * kLrSlots), 0, s, slots, counts);
    return hipGetLastError();
}

hipError_t launch_lr_fill(const LrMaps &m, hipStream_t s)
{
    hipLaunchKernelGGL(ws_lr_fill_kernel, dim3((unsigned)(m.h[0] + m.h[1])), dim3(kLrThreads), 0, s, m);
    return hipGetLastError();
}

} // namespace wsamd
