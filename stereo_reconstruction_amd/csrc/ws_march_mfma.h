// ws_march_mfma.h -- the SSD search with its cross term on the int8 matrix cores (device code; instantiated by
// ws_march_mfma.hip).  The stencil kernel (ws_march_kernel.h) spends 4.5 of its 6 instructions per hypothesis on forming
// sum a.b over the window and sliding it down the strip; that sum is a contraction:
//
//   sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a.b,     a^ = a xor 0x80, b^ = b xor 0x80 read as signed bytes (a - 128):
//   (a - b) = (a^ - b^), so the costs are unchanged and every operand is an int8.
//
//   * The window of ONE row is 3 * WW contiguous bytes of the caller's BGR row: for output column x the bytes from
//     3 (x + wx0) on, for target centre column v the bytes from 3 (v + wx0) on.  R(y; x, v) = sum_k a^[k] b^[k] is a GEMM
//     with K = 3 WW padded to 32 (the pad zeroed on the A side only): M = 32 consecutive v, N = 32 consecutive x, one
//     v_mfma_i32_32x32x32_i8.  No im2col pass: the raw rows in LDS are the im2col matrix at a stride of 3 bytes per row.
//   * N (the lane) is x, M (the accumulator registers) is v: a lane holds 16 candidates of ITS OWN output pixel per
//     tile, the argmin over d needs no cross-lane traffic but one exchange between the two lane halves.
//   * The accumulator slides: per step and tile two MFMAs into the same accumulator -- the entering row with the A side
//     complemented (~a^ = -a^ - 1), the leaving row plain:  Acc += -R(e) - T(e, v) + R(l),  T(y, v) = sum_k b^[y][k].
//     After any number of steps Acc = -(cross sum over the window's rows) - E(v), E(v) = sum of T over every row entered.
//   * key = (Acc << (KT + 1)) + bias'[v],  bias'[v] = ((window sum of b^^2) + 2 E(v)) << KT | tie tag, poisoned where the
//     target centre is invalid; all modulo 2^32, the key exact.  Candidates outside [d_lo, d_hi] are poisoned through the
//     accumulator's initial value (kPoison >> (KT + 1)), which costs nothing per step.
//   * v_min3 over a tile's 16 registers (4-bit tags: register order is disparity order), a strict '<' between tiles taken
//     in the preferred order of d, and one exchange between lane n and lane n + 32.
//
// Geometry: a workgroup of 8 waves owns a tile of 128 columns and a strip of rows; two waves share columns 32 wx .. 32 wx + 31
// and split their NV tiles of 32 target centres (NV = 9 covers 256 disparities) 5 : 4, each with its 16 accumulators per
// tile in registers for the whole strip; the second wave hands its best candidate to the first through LDS, which writes
// the row out one step later.
// Rows travel HBM -> LDS as the bytes they are (raw_dma of ws_march_kernel.h) into a ring of WH + 4 raw rows per
// image, three stages ahead of their use, one barrier per step:
//   step s:  copy row s + 3  |  xor row s + 2 with 0x80 in place  |  row s + 1: bias' values, the target row as lane-linear
//            MFMA operands (a ring of WH + 2 rows of 12 KB)  |  MFMAs, keys of row s, output of row s - 1.
#pragma once
#include "ws_march_kernel.h"

namespace wsamd {

typedef int ws_i32x4 __attribute__((ext_vector_type(4)));
typedef int ws_i32x16 __attribute__((ext_vector_type(16)));
typedef int ws_i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) ws_i32x2 lds_i64;

constexpr int kMfmaXWaves = 4; // waves side by side: 128 columns per tile
constexpr int kMfmaVWaves = 2; // waves that share 32 columns and split their candidates
constexpr int kMfmaWaves = kMfmaXWaves * kMfmaVWaves;
constexpr int kMfmaVTiles = 9; // tiles of 32 target centres per 32 columns: 32 + 255 candidate columns -> up to 256 disparities
constexpr int kMfmaTilesPerWave = (kMfmaVTiles + kMfmaVWaves - 1) / kMfmaVWaves;
constexpr int kMfmaKT = 4;     // tie-tag bits: the 16 registers of a tile

struct MfmaLds {
    int n_a, n_b;   // pixels per raw row the copies fetch
    int rb_a, rb_b; // bytes per raw row buffer
    int nvc;        // target centres per tile row (bias values)
    int o_b, o_bias, o_merge, o_op;
    int nblk; // blocks of 32 target centres per tile row
    int bytes;
};
__host__ __device__ constexpr int mfma_ring_rows(int wh) { return wh + 4; }
__host__ __device__ constexpr int mfma_op_rows(int wh) { return wh + 2; } // rows s + 1 (being written) .. s - wh
__host__ __device__ inline MfmaLds mfma_lds_layout(int ww, int wh)
{
    MfmaLds l{};
    const int tx = 32 * kMfmaXWaves;
    l.nvc = tx + 32 * (kMfmaVTiles - 1);
    // a lane reads 32 bytes from its column's first byte on (the pad beyond 3 WW is multiplied by zero), 5 dwords at a time
    l.n_a = tx + 12;
    l.n_b = l.nvc + 12;
    l.rb_a = march_raw_bytes(l.n_a);
    l.rb_b = march_raw_bytes(l.n_b);
    l.o_b = mfma_ring_rows(wh) * l.rb_a;
    l.o_bias = l.o_b + mfma_ring_rows(wh) * l.rb_b;
    l.o_merge = l.o_bias + 2 * 4 * l.nvc;
    l.o_op = l.o_merge + 2 * 8 * tx; // (two rows of (cost word, candidate) per column)
    l.nblk = l.nvc / 32;
    l.bytes = l.o_op + mfma_op_rows(wh) * l.nblk * 1024; // the target rows as MFMA operands: 64 lanes x 16 bytes per block
    (void)ww;
    return l;
}

// 16 bytes from LDS byte address row + p (any alignment): 5 dwords, 4 v_alignbyte
__device__ __forceinline__ ws_i32x4 mfma_operand(uint32_t row, uint32_t p)
{
    const lds_u32 *q = lds_at32(row + (p & ~3u));
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
    const uint32_t sh = p & 3u;
    ws_i32x4 r;
    r.x = (int)__builtin_amdgcn_alignbyte(d1, d0, sh);
    r.y = (int)__builtin_amdgcn_alignbyte(d2, d1, sh);
    r.z = (int)__builtin_amdgcn_alignbyte(d3, d2, sh);
    r.w = (int)__builtin_amdgcn_alignbyte(d4, d3, sh);
    return r;
}

template <int WW, int WH>
__global__ void __launch_bounds__(64 * kMfmaWaves) ws_march_mfma_kernel(const MarchArgs g)
{
    constexpr int NW = kMfmaWaves, NV = kMfmaVTiles, NVW = kMfmaTilesPerWave, KT = kMfmaKT, NT = 64 * NW, TX = 32 * kMfmaXWaves;
    constexpr int NR = mfma_ring_rows(WH);
    constexpr int K = 3 * WW;
    static_assert(K <= 32 && K > 16, "one row of the window is one K = 32 step, its pad in the upper lane half");
    static_assert(TX + 32 * (NV - 1) <= NT, "one bias value per thread");
    // a centred cost word sum b^^2 - 2 sum a^.b^ lies in [-128^2, 128^2 + 2 * 127 * 128] per byte of the window
    static_assert((long long)(128 * 128 + 2 * 127 * 128) * K * WH * (1 << KT) < (long long)kValidKeyBound, "keys stay inside (-2^28, 2^28)");
    static_assert(kPoison % (1 << (KT + 1)) == 0, "the poison survives the shift");

    extern __shared__ uint4 ws_smem4[];
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_u32 *)reinterpret_cast<uint32_t *>(ws_smem4);
    const MfmaLds L = mfma_lds_layout(WW, WH);
    const uint32_t RBA = (uint32_t)L.rb_a, RBB = (uint32_t)L.rb_b;
    const uint32_t ringA = lds0, ringB = lds0 + (uint32_t)L.o_b, biasr = lds0 + (uint32_t)L.o_bias, mrg = lds0 + (uint32_t)L.o_merge;
    const uint32_t opB = lds0 + (uint32_t)L.o_op, OPROW = 1024u * (uint32_t)L.nblk;
    constexpr int NRO = mfma_op_rows(WH);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    const int wx = wave & (kMfmaXWaves - 1), wv = wave >> 2; // this wave's 32 columns, its share of their tiles: t = wv NVW + j
    static_assert(kMfmaXWaves == 4, "wave >> 2");

    const int nblk = gridDim.x; // padded to a multiple of 8 by the launcher: every XCD a contiguous range of (strip, tile) pairs
    const int logical = (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3);
    if (logical >= g.tiles * g.strips) return;
    const int tile_i = logical % g.tiles, strip_i = logical / g.tiles;
    const int tile_x0 = g.ox0 + tile_i * TX;
    const int ys = g.oy0 + strip_i * g.strip_rows;
    const int ye = min(ys + g.strip_rows, g.oy1);
    if (ys >= ye) return;

    // left view: the map's pixels outside the marching interior are zeros; the tiles along the interior's edge write them
    if (g.border) {
        const bool first_t = tile_i == 0, last_t = tile_i == g.tiles - 1;
        const int cx0 = first_t ? 0 : tile_x0, cx1 = last_t ? g.out_w : tile_x0 + TX;
        auto zero_rect = [&](int x0, int x1, int y0, int y1) __attribute__((always_inline)) {
            const int w = x1 - x0, cnt = w * (y1 - y0);
            for (int i = tid; i < cnt; i += NT) {
                const int yy = y0 + i / w, xx = x0 + i % w;
                if (g.out16) g.out16[(size_t)yy * g.out_pitch + xx] = 0;
                else g.out[(size_t)yy * g.out_pitch + xx] = 0.0f;
            }
        };
        if (strip_i == 0 && g.oy0 > 0) zero_rect(cx0, cx1, 0, g.oy0);
        if (strip_i == g.strips - 1 && g.out_h > g.oy1) zero_rect(cx0, cx1, g.oy1, g.out_h);
        if (first_t && g.ox0 > 0) zero_rect(0, g.ox0, ys, ye);
        if (last_t && g.out_w > g.ox1) zero_rect(g.ox1, g.out_w, ys, ye);
    }

    // the rings start as zeros: bytes outside the image are never copied, and whatever they hold they hold for a row's
    // whole life (the candidates that read them are poisoned, their keys stay bounded because they are bytes)
    for (int k = tid; k < L.o_bias / 16; k += NT) lds_store128(lds0 + 16u * (uint32_t)k, make_uint4(0u, 0u, 0u, 0u));

    const int dspan = g.d_hi - g.d_lo;
    // raw index 0 of ring A is image column tile_x0 + wx0; of ring B the first byte of target centre vb0's window,
    // vb0 = the centre of bias index 0: candidate (x, v) has d = d_lo + 32 (NV - 1) + (x - tile_x0) - (v - vb0)
    const int vb0 = tile_x0 + g.st.boff - g.d_lo - 32 * (NV - 1);
    const int ra0 = ys + g.wy0;
    const int nsteps = (ye - ys) + WH - 1;
    const RawSide sideA = raw_side(g.st.img_a, g.st.stride_a, g.st.wa, tile_x0 + g.st.wx0, L.n_a, 0);
    const RawSide sideB = raw_side(g.st.img_b, g.st.stride_b, g.st.wb, vb0 + g.st.wx0, L.n_b, 0);
    const RawDma dmaMine = raw_dma_setup(wave == 0 ? sideA : sideB, ra0);
    const uint32_t phA0 = (uint32_t)(reinterpret_cast<uintptr_t>(sideA.base) + (uintptr_t)((long long)ra0 * sideA.stride + 3LL * sideA.c0)) & 15u;
    const uint32_t phB0 = (uint32_t)(reinterpret_cast<uintptr_t>(sideB.base) + (uintptr_t)((long long)ra0 * sideB.stride + 3LL * sideB.c0)) & 15u;
    const uint32_t stA = (uint32_t)sideA.stride & 15u, stB = (uint32_t)sideB.stride & 15u;
    // strip row i (any i >= -NR): its ring slot and the byte phase of raw index 0 in it
    auto slot_of = [&](int i) __attribute__((always_inline)) { return (uint32_t)(i + NR) % (uint32_t)NR; };
    auto opslot_of = [&](int i) __attribute__((always_inline)) { return (uint32_t)(i + 2 * NRO) % (uint32_t)NRO; };
    auto phase_a = [&](int i) __attribute__((always_inline)) { return (phA0 + (uint32_t)i * stA) & 15u; };
    auto phase_b = [&](int i) __attribute__((always_inline)) { return (phB0 + (uint32_t)i * stB) & 15u; };

    // ---- this thread's bias value: target centre vb0 + tid ----------------------------------------------------
    // tag: register i of a tile holds row m = (i & 3) + 8 (i >> 2) + 4 h of it; smaller m = larger d = preferred
    const int bm = tid & 31;
    const bool bvalid = (uint32_t)(vb0 + tid - g.st.b_lo) <= (uint32_t)(g.st.b_hi - g.st.b_lo) && g.st.b_hi >= g.st.b_lo;
    const uint32_t btag = (uint32_t)((bm & 3) + 4 * (bm >> 3)) + (bvalid ? 0u : (uint32_t)kPoison);
    uint32_t gsum = 0u; // (window sum of b^^2) + 2 E, modulo 2^32

    // ---- the accumulators ---------------------------------------------------------------------------------------
    // tile t, register i: e = d - d_lo = 32 (NV - 1 - t) + n - m; outside [0, dspan]: poisoned for good
    ws_i32x16 acc[NVW];
    uint32_t active = 0u; // this wave's tiles with a valid candidate (a narrow range skips the others' MFMAs)
#pragma unroll
    for (int j = 0; j < NVW; ++j) {
        const int t = wv * NVW + j;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = (i & 3) + 8 * (i >> 2) + 4 * h;
            const int e = 32 * (NV - 1 - t) + n - m;
            acc[j][i] = (uint32_t)e <= (uint32_t)dspan ? 0 : kPoison >> (KT + 1);
        }
        if (t < NV && 32 * (NV - 1 - t) - 31 <= dspan) active |= 1u << j; // (its smallest e is within the range; 31 >= 0 always is)
    }
    const uint32_t all_tiles = (1u << min(NVW, NV - wv * NVW)) - 1u; // this wave's share of the tiles
    const bool wave_on = tile_x0 + 32 * wx < g.ox1; // (a wave all of whose columns lie past the interior only helps with the stages)

    // pad mask of the A operand: bytes K .. 31 of the 32 a lane pair holds are zero (h = 1 holds bytes 16 .. 31)
    ws_i32x4 amask;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int first = 16 * h + 4 * j; // this dword's first byte
        const int keep = K - first;       // bytes of it inside the window
        amask[j] = keep >= 4 ? -1 : keep <= 0 ? 0 : (int)((1u << (8 * keep)) - 1u);
    }
    const uint32_t pA_lane = 3u * (uint32_t)(32 * wx + n) + 16u * (uint32_t)h; // byte of this lane's operand part in a raw A row
    const uint32_t opB_lane = 1024u * (uint32_t)(wx + wv * NVW) + 16u * (uint32_t)lane; // ... in an operand row of B, tile j of this wave: + 1024 j

    __syncthreads();

    int my_cw = 0, my_G = 0; // the first wave's own best of the last step
    // the output row of step sp: the better of the two waves' candidates, the fallback, the black-pixel rule
    auto flush = [&](int sp) __attribute__((always_inline)) {
        if (wv != 0 || !wave_on) return;
        const ws_i32x2 o = *reinterpret_cast<const lds_i64 *>((uintptr_t)(mrg + 8u * (uint32_t)((sp & 1) * TX + 32 * wx + n)));
        int cw = my_cw, G = my_G;
        if (o.x < cw || (o.x == cw && o.y < G)) { cw = o.x; G = o.y; }
        const int oi = sp - (WH - 1);
        const int x = tile_x0 + 32 * wx + n, y = ys + oi;
        if (h == 0 && x < g.ox1) {
            float val;
            if (cw >= (kValidKeyBound >> KT)) val = g.fallback_neg ? -(float)x : (float)x; // no valid candidate
            else val = (float)(g.d_lo + 32 * (NV - 1) + n - G);
            // black pixel: image row y is strip row oi - wy0, column x raw index 32 wx + n - wx0 of ring A
            const int ic = oi - g.wy0;
            const uint32_t p = phase_a(ic) + 3u * (uint32_t)(32 * wx + n - g.st.wx0);
            const lds_u32 *q = lds_at32(ringA + slot_of(ic) * RBA + (p & ~3u));
            const uint32_t px = __builtin_amdgcn_alignbyte(q[1], q[0], p & 3u) & 0x00ffffffu;
            if (px == kCentre) val = 0.0f;
            if (g.out16) g.out16[(size_t)y * g.out_pitch + x] = (int16_t)(int)val;
            else g.out[(size_t)y * g.out_pitch + x] = val;
        }
    };

    auto step = [&](int s, auto phase) __attribute__((always_inline)) {
        // PHASE -1: the stages alone, 0: rows enter, 1: the strip's first output row, 2: a row enters, a row leaves
        constexpr int PHASE = decltype(phase)::value;
        if constexpr (PHASE == 2) flush(s - 1);
        // 1. copy row s + 3 (wave 0: image A, wave 1: image B)
        if (wave < 2 && s + 3 < nsteps) {
            const uint32_t sl = slot_of(s + 3);
            raw_dma(wave == 0 ? ringA + sl * RBA : ringB + sl * RBB, dmaMine, s + 3, lane);
        }
        // 2. row s + 2 landed in the last step: centre its bytes
        if (s + 2 >= 0 && s + 2 < nsteps) {
            const uint32_t sl = slot_of(s + 2);
            const int na16 = (int)(RBA >> 4), nb16 = (int)(RBB >> 4);
            for (int k = tid; k < na16 + nb16; k += NT) {
                const uint32_t at = k < na16 ? ringA + sl * RBA + 16u * (uint32_t)k : ringB + sl * RBB + 16u * (uint32_t)(k - na16);
                uint4 v = lds_load128(at);
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                lds_store128(at, v);
            }
        }
        // 3. the bias value of this thread's target centre for step s + 1: row s + 1 enters, row s + 1 - WH leaves
        if (s + 1 >= 0 && s + 1 < nsteps && tid < L.nvc) {
            const int iu = s + 1;
            constexpr int NDW = (K + 3) / 4; // dwords that hold a window's K bytes
            auto window = [&](int i, uint32_t (&d)[NDW]) __attribute__((always_inline)) {
                const uint32_t p = phase_b(i) + 3u * (uint32_t)tid;
                const lds_u32 *q = lds_at32(ringB + slot_of(i) * RBB + (p & ~3u));
                uint32_t r[NDW + 1];
#pragma unroll
                for (int j = 0; j < NDW + 1; ++j) r[j] = q[j];
#pragma unroll
                for (int j = 0; j < NDW; ++j) {
                    d[j] = __builtin_amdgcn_alignbyte(r[j + 1], r[j], p & 3u);
                    const int keep = K - 4 * j;
                    if (keep < 4) d[j] &= (1u << (8 * keep)) - 1u; // (the centred bytes past the window count as zeros)
                }
            };
            uint32_t d[NDW];
            window(iu, d);
#pragma unroll
            for (int j = 0; j < NDW; ++j) {
                gsum = (uint32_t)__builtin_amdgcn_sdot4((int)d[j], (int)d[j], (int)gsum, false);
                gsum += 2u * (uint32_t)__builtin_amdgcn_sdot4((int)d[j], 0x01010101, 0, false);
            }
            if (iu >= WH) {
                window(iu - WH, d);
                uint32_t lq = 0u;
#pragma unroll
                for (int j = 0; j < NDW; ++j) {
                    lq = (uint32_t)__builtin_amdgcn_sdot4((int)d[j], (int)d[j], (int)lq, false);
                }
                gsum -= lq;
            }
            *reinterpret_cast<lds_u32 *>((uintptr_t)(biasr + 4u * (uint32_t)((iu & 1) * L.nvc + tid))) = (gsum << KT) + btag;
        }
        // 4. row s + 1 of the target image as MFMA operands: per block of 32 target centres 64 lanes x 16 bytes, lane-linear,
        //    so that the waves that multiply it -- up to 8 per block, when it enters and again when it leaves -- read one
        //    aligned ds_read_b128 each instead of assembling it from the raw bytes
        if (s + 1 >= 0 && s + 1 < nsteps) {
            const uint32_t rowB = ringB + slot_of(s + 1) * RBB, dst = opB + opslot_of(s + 1) * OPROW, phb = phase_b(s + 1);
            for (int k = tid; k < 64 * L.nblk; k += NT) { // (whole waves: k >> 6 is the block)
                const ws_i32x4 v = mfma_operand(rowB, phb + 3u * (uint32_t)(32 * (k >> 6) + n) + 16u * (uint32_t)h);
                lds_store128(dst + 16u * (uint32_t)k, make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w));
            }
        }
        // 5. the matrix cores: row s enters every window, row s - WH leaves it; keys and the output row
        if constexpr (PHASE >= 0) {
            if (wave_on) {
                const uint32_t rowAe = ringA + slot_of(s) * RBA, rowAl = ringA + slot_of(s - WH) * RBA;
                const uint32_t pae = phase_a(s) + pA_lane, pal = phase_a(s - WH) + pA_lane;
                const uint32_t opBe = opB + opslot_of(s) * OPROW + opB_lane, opBl = opB + opslot_of(s - WH) * OPROW + opB_lane;
                ws_i32x4 ae = mfma_operand(rowAe, pae), al;
                ae = ~ae & amask; // (the complement first, then the pad: it must stay zero)
                if constexpr (PHASE == 2) al = mfma_operand(rowAl, pal) & amask;
                int bestk = INT_MAX, bestt = 0;
                const uint32_t brow = biasr + 4u * (uint32_t)((s & 1) * L.nvc + 32 * (wx + wv * NVW) + 4 * h);
                // (all of a wave's tiles active -- the usual case -- is a loop without branches: the compiler then overlaps
                // the tiles' operand reads, MFMAs and keys; a narrow range takes the loop that skips tiles)
                auto tiles = [&](auto all) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < NVW; ++t) { // (t: the tile's index in this wave)
                    if constexpr (!decltype(all)::value || (NV % NVW != 0)) { // (the second wave's share is one tile short)
                        if ((!decltype(all)::value || t == NVW - 1) && !(active & (1u << t))) continue; // (uniform)
                    }
                    const uint4 be4 = lds_load128(opBe + 1024u * (uint32_t)t);
                    const ws_i32x4 be = {(int)be4.x, (int)be4.y, (int)be4.z, (int)be4.w};
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(be, ae, acc[t], 0, 0, 0);
                    if constexpr (PHASE == 2) {
                        const uint4 bl4 = lds_load128(opBl + 1024u * (uint32_t)t);
                        const ws_i32x4 bl = {(int)bl4.x, (int)bl4.y, (int)bl4.z, (int)bl4.w};
                        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bl, al, acc[t], 0, 0, 0);
                    }
                    if constexpr (PHASE >= 1) {
                        int key[16];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint4 b4 = lds_load128(brow + 4u * (uint32_t)(32 * t + 8 * q));
                            key[4 * q + 0] = (int)(((uint32_t)acc[t][4 * q + 0] << (KT + 1)) + b4.x);
                            key[4 * q + 1] = (int)(((uint32_t)acc[t][4 * q + 1] << (KT + 1)) + b4.y);
                            key[4 * q + 2] = (int)(((uint32_t)acc[t][4 * q + 2] << (KT + 1)) + b4.z);
                            key[4 * q + 3] = (int)(((uint32_t)acc[t][4 * q + 3] << (KT + 1)) + b4.w);
                        }
                        int km = min(key[0], key[1]);
#pragma unroll
                        for (int i = 2; i < 16; i += 2) km = min(km, min(key[i], key[i + 1])); // v_min3_i32
                        // a later tile (smaller d) wins on a strictly smaller cost only
                        const bool better = (km | ((1 << KT) - 1)) < bestk;
                        bestk = better ? km : bestk;
                        bestt = better ? t : bestt;
                    }
                }
                };
                if (active == all_tiles) tiles(std::true_type());
                else tiles(std::false_type());
                if constexpr (PHASE >= 1) {
                    // the two halves of a column: G = 32 t + m orders ALL its candidates (smaller = larger d)
                    const int i_best = bestk & ((1 << KT) - 1);
                    int G = 32 * (bestt + wv * NVW) + (i_best & 3) + 8 * (i_best >> 2) + 4 * h;
                    int cw = bestk >> KT; // the cost word
                    const int cw_o = __shfl_xor(cw, 32, 64), G_o = __shfl_xor(G, 32, 64);
                    if (cw_o < cw || (cw_o == cw && G_o < G)) { cw = cw_o; G = G_o; }
                    // the second wave of a column leaves its best in LDS for the first, which writes the row out in the next step
                    if (wv == 1) {
                        if (h == 0) *reinterpret_cast<lds_i64 *>((uintptr_t)(mrg + 8u * (uint32_t)((s & 1) * TX + 32 * wx + n))) = ws_i32x2{cw, G};
                    } else {
                        my_cw = cw;
                        my_G = G;
                    }
                }
            }
        }
        if (wave < 2) dma_wait();
        __syncthreads();
    };

    int s = -3;
#pragma unroll 1
    for (; s < 0; ++s) step(s, std::integral_constant<int, -1>());
#pragma unroll 1
    for (; s < WH - 1; ++s) step(s, std::integral_constant<int, 0>());
    step(s++, std::integral_constant<int, 1>());
#pragma unroll 1
    for (; s < nsteps; ++s) step(s, std::integral_constant<int, 2>());
    flush(nsteps - 1); // the last row
}

} // namespace wsamd
