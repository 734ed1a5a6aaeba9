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
//     target centre is invalid.  KT = 3, so the shift is 4 and the keys of an aligned register pair are ONE
//     v_lshl_add_u64 on the pair and its two bias words; accumulators and bias words carry uniform offsets that keep
//     every word non-negative and every sum inside its word (kMfmaA0 .. below), the key exact and compared unsigned.
//     Candidates outside [d_lo, d_hi] are poisoned through the accumulator's initial value, which costs nothing per step.
//   * per tile two chains of v_min3_u32, over the low and the high words of the 8 pairs (3-bit tags: the pair's index,
//     register order is disparity order), a compare between the chains, a strict '<' between tiles taken in the
//     preferred order of d, and one exchange between lane n and lane n + 32.
//
// Geometry: a workgroup of 8 waves owns a tile of 128 columns and a strip of rows; two waves share columns 32 wx .. 32 wx + 31
// and split their NV tiles of 32 target centres (NV = 9 covers 256 disparities) 5 : 4, each with its 16 accumulators per
// tile in registers for the whole strip; the first wave hands its best candidate to the second through LDS, which writes
// the row out one step later.
// Rows travel HBM -> LDS as the bytes they are (raw_dma of ws_march_kernel.h) into a ring of WH + 4 raw rows per
// image, and stay raw: every consumer centres the bytes in an instruction it issues anyway.  One barrier per step:
//   step s:  copy row s + 3  |  (row s + 2 rests: the copies' look-ahead)  |  row s + 1 of the target image: its
//            lane-linear MFMA operands (a ring of WH + 2 rows of 12 KB; a block of 32 centres is 4 v_alignbyte and 4
//            v_bitop3, centred and masked, on a lane pair per centre) and its bias' values: the sums over a centre's
//            window bytes are a box over per-pixel sums, formed once per pixel -- a lane a pixel, the neighbours' by
//            DPP -- and not once per centre that holds the pixel (the window's sum of squares stays in the pad of the
//            centre's operand entry and is read back, not computed again, when the row leaves the windows)  |  MFMAs,
//            keys of row s, output of row s - 1.
// The step ends when its slowest wave reaches the barrier, so the roles are dealt by tile share: the waves with 5 tiles
// (wv = 0) take one block of operands each and waves 0 and 1 the copies, the waves with 4 tiles (wv = 1) take two blocks
// each, the merge of the two waves' candidates and the store of the output row; every wave takes one chunk of 58
// centres' sums.  A wave's role is a template argument of its march, the rows' ring offsets and byte phases are
// scalars advanced with a compare and a wrap, and the steady phase of a strip has no guard.
//
// The steady step (PHASE 2, and the tile loop of PHASE 3) of the march with every tile active is a software pipeline,
// pinned with __builtin_amdgcn_sched_barrier / sched_group_barrier because source order alone does not survive the
// scheduler (tools/mfma_listing.py prints what came out; profiles/mfma_pipeline/README.md holds the tables):
//   1. what the step reads and the step before it does not write -- the two raw A rows, the NTL operand quads of the
//      leaving row, the operand pass's rows -- is read a tile's keys ahead of the barrier of the step BEFORE
//      (ahead_load; the cursors advance in the middle of a step, behind their last use), so it has landed when the
//      barrier opens.  Behind the barrier only the NTL operand quads of the entering row and the bias quads of tile 0
//      are read, together, ahead of the first wait.  LDS returns in issue order, so each wait is a counted lgkmcnt(N)
//      that covers what the next instruction consumes and nothing younger;
//   2. the entering MFMAs of all tiles, then the leaving MFMAs, in four groups (entering 0 .. NTL - 3 | NTL - 2,
//      NTL - 1 | leaving 0, 1 | then one leaving MFMA per key block): inside a group the compiler may take any order,
//      and no order puts two MFMAs on one accumulator side by side.  The operand pass's VALU (a block's operands:
//      items_enter; a chunk's sums in two halves: sums_box, sums_leave) sits between the MFMAs of the first three groups;
//   3. tile t's keys and minimum run under the leaving MFMA of tile t + 2; the bias quads of tile t + 1 (a double
//      buffer of 2 x 16 registers) are read a whole key block ahead of their use.  The minimum of the 16 keys is two
//      chains of 8, min(min(km, a), b): one v_min and 3 v_min3 each (mfma_tile_best);
//   4. the two lane halves of a column meet in two v_permlane32_swap and a compare / select (mfma_pair_best): no LDS
//      round trip and no branch in front of the barrier.
// The march that skips tiles (a narrow disparity range) and the phases before the first leaving row keep the simple
// tile loop.  The flush is where it was: the merge pair it reads is written by the partner wave in the step before, so
// it is read behind the barrier, first of all reads; flush_store follows the half merge.  What each item measured, and
// what was dropped (a static s_setprio for the 4-tile waves: slower): profiles/mfma_pipeline/README.md.
#pragma once
#include "ws_march_kernel.h"

namespace wsamd {

typedef int ws_i32x4 __attribute__((ext_vector_type(4)));
typedef int ws_i32x16 __attribute__((ext_vector_type(16)));
typedef int ws_i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) ws_i32x2 lds_i64;
typedef unsigned long long ws_u64x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long ws_u64x2 __attribute__((ext_vector_type(2)));

constexpr int kMfmaXWaves = 4; // waves side by side: 128 columns per tile
constexpr int kMfmaVWaves = 2; // waves that share 32 columns and split their candidates
constexpr int kMfmaWaves = kMfmaXWaves * kMfmaVWaves;
constexpr int kMfmaVTiles = 9; // tiles of 32 target centres per 32 columns: 32 + 255 candidate columns -> up to 256 disparities
constexpr int kMfmaTilesPerWave = (kMfmaVTiles + kMfmaVWaves - 1) / kMfmaVWaves;
constexpr int kMfmaKT = 3;     // tie-tag bits: the 8 register pairs of a tile

// ---- the key's ranges ------------------------------------------------------------------------------------------------
// Two keys come out of one v_lshl_add_u64 on an aligned register pair, (Acc << 4) + bias' on 64 bits, so nothing may
// cross from the low word into the high one: the 4 bits shifted out of the low accumulator are zeros and the low sum
// does not carry.  Accumulators and bias words are therefore kept non-negative by uniform offsets, and every bound
// follows from the longest strip the kernel is taken for, kMfmaMaxSteps rows entered (the launcher's rule refuses
// longer ones).  For a window of K bytes per row and WH rows, centred bytes in [-128, 127]:
//   |cross sum| <= XB = 128^2 K WH,   |E(v)| <= EB = 128 K kMfmaMaxSteps,   0 <= window sum of b^^2 <= XB,
//   Acc = -(cross sum) - E in [-(XB + EB), XB + EB],   gsum = (sum of b^^2) + 2 E in [-2 EB, XB + 2 EB],
//   cost word 2 Acc + gsum = (sum of b^^2) - 2 (cross sum) in [-2 XB, 3 XB]   (E cancels).
// Acc starts at kMfmaA0 (+ kMfmaAccPoison outside [d_lo, d_hi]), gsum at kMfmaG0 (+ kMfmaBiasPoison at an invalid
// centre); the cost word carries kMfmaC0 = 2 A0 + G0, the same for every candidate, so their order is what it was.
constexpr int kMfmaMaxSteps = 8192;
constexpr long long kMfmaA0 = 1LL << 25, kMfmaAccPoison = 1LL << 27;
constexpr long long kMfmaG0 = 1LL << 26, kMfmaBiasPoison = 1LL << 26;
constexpr long long kMfmaC0 = 2 * kMfmaA0 + kMfmaG0;
constexpr long long kMfmaValidBound = kMfmaC0 + (1LL << 25); // a cost word at or above it holds a poison
template <int K, int WH>
constexpr bool mfma_key_ranges_hold()
{
    constexpr long long XB = 128LL * 128 * K * WH, EB = 128LL * K * kMfmaMaxSteps;
    static_assert(XB + EB < kMfmaA0, "Acc + A0 stays positive");
    static_assert(kMfmaA0 + XB + EB + kMfmaAccPoison < (1LL << 28), "the 4 bits shifted out of an accumulator are zeros");
    static_assert(2 * EB <= kMfmaG0, "gsum + G0 stays non-negative");
    static_assert(((kMfmaG0 + XB + 2 * EB + kMfmaBiasPoison) << kMfmaKT) + (1 << kMfmaKT) <= (1LL << 31), "a bias word is a positive int");
    static_assert(kMfmaC0 - 2 * XB >= 0, "a cost word is positive");
    static_assert(((kMfmaC0 + 3 * XB + 2 * kMfmaAccPoison + kMfmaBiasPoison) << kMfmaKT) + (1 << kMfmaKT) <= (1LL << 32),
                  "a doubly poisoned key does not wrap, and the low word of a pair does not carry");
    static_assert(kMfmaC0 + 3 * XB < kMfmaValidBound, "every valid cost word is below the bound");
    static_assert(kMfmaC0 - 2 * XB + 2 * kMfmaAccPoison >= kMfmaValidBound && kMfmaC0 - 2 * XB + kMfmaBiasPoison >= kMfmaValidBound,
                  "every poisoned cost word is at or above it");
    return true;
}

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

// 16 bytes from LDS byte address t (any alignment): 5 dword reads now, 4 v_alignbyte when the bytes are needed
struct MfmaRaw {
    uint32_t d0, d1, d2, d3, d4, sh;
};
__device__ __forceinline__ MfmaRaw mfma_raw_load(uint32_t t)
{
    const lds_u32 *q = lds_at32(t & ~3u);
    return MfmaRaw{q[0], q[1], q[2], q[3], q[4], t & 3u};
}
__device__ __forceinline__ ws_i32x4 mfma_raw_align(const MfmaRaw &r)
{
    ws_i32x4 v;
    v.x = (int)__builtin_amdgcn_alignbyte(r.d1, r.d0, r.sh);
    v.y = (int)__builtin_amdgcn_alignbyte(r.d2, r.d1, r.sh);
    v.z = (int)__builtin_amdgcn_alignbyte(r.d3, r.d2, r.sh);
    v.w = (int)__builtin_amdgcn_alignbyte(r.d4, r.d3, r.sh);
    return v;
}

// lane n and lane n + 32 both get the better of their two candidates (smaller cost word, then smaller G): two
// v_permlane32_swap, no LDS, no branch
__device__ __forceinline__ void mfma_pair_best(int &cw, int &G)
{
    const auto c = __builtin_amdgcn_permlane32_swap((uint32_t)cw, (uint32_t)cw, false, false); // {lane n's, lane n + 32's} in both lanes
    const auto q = __builtin_amdgcn_permlane32_swap((uint32_t)G, (uint32_t)G, false, false);
    const int c0 = (int)c[0], c1 = (int)c[1], g0 = (int)q[0], g1 = (int)q[1];
    const bool up = c1 < c0 || (c1 == c0 && g1 < g0);
    cw = up ? c1 : c0;
    G = up ? g1 : g0;
}

// The sizes of the VALU groups that sched_group_barrier places behind the MFMAs of the steady step.  They are read off
// the gfx950 listing, not derived: kPipeValuA = the instructions that make the entering row's A operand in front of
// the first MFMA (4 v_alignbyte + 4 v_bitop3); kPipeValu[role] = the VALU of the operand pass that lies between the
// first six MFMAs divided by the MFMAs it is spread under, rounded up: a block's operands are 8 instructions and its
// addresses, a chunk's packed window sums 11, its running sum and bias word 9 -- 12 under two MFMAs at the most, on
// either role.  A group asks for "up to" its size, so a number that is off, or another compiler's instruction count,
// regroups the VALU and changes no result; after a toolchain change tools/mfma_listing.py is the check (no
// neighbouring MFMAs on one accumulator, the read-to-wait distances).
constexpr int kPipeValuA = 8;
constexpr int kPipeValu[2] = {6, 6};

// The keys of a tile and their minimum.  Registers 2 q, 2 q + 1 and their two bias words are aligned 64-bit pairs, and
// (Acc << 4) + bias' on the pair is both keys (kMfmaKT above: nothing crosses between the words): 8 v_lshl_add_u64.  The
// tag of a key is its pair's index q, so the minimum runs in two chains, L over the low words (registers 0, 2, .. 14)
// and H over the high words (1, 3, .. 15), one v_min and three v_min3_u32 each.  Inside a chain the tags order equal
// costs; between them H wins exactly when kmH < kmL as integers: on equal cost register 2 qH + 1 is preferred over
// 2 qL exactly when qH < qL.  Between tiles a later tile (smaller d) wins on a strictly smaller cost only.
// The tile-level chain keeps the best key, its tile and the L minimum of that tile: the key is min(kmL, kmH), so H won
// exactly where it differs from the L minimum, which is asked once behind the last tile (mfma_best_code: 2 t + isH)
// and costs one select per tile.  FIRST: no tile before this one (the best so far is "none").
struct MfmaBest {
    uint32_t k, l, t;
};
__device__ __forceinline__ uint32_t mfma_best_code(const MfmaBest &b) { return 2u * b.t + (b.k < b.l ? 1u : 0u); }
template <bool FIRST>
__device__ __forceinline__ void mfma_tile_best(const ws_i32x16 &acc, const uint4 (&b4)[4], int t, MfmaBest &best)
{
    const ws_u64x8 a = __builtin_bit_cast(ws_u64x8, acc);
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const ws_u64x2 b = __builtin_bit_cast(ws_u64x2, b4[q]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // (plain C++, not inline assembly: the compiler must see a VALU read of an MFMA result to keep its distance)
            const unsigned long long k = (a[2 * q + j] << (kMfmaKT + 1)) + b[j];
            lo[2 * q + j] = (uint32_t)k, hi[2 * q + j] = (uint32_t)(k >> 32);
        }
    }
    uint32_t kl = min(lo[0], lo[1]), kh = min(hi[0], hi[1]);
#pragma unroll
    for (int q = 2; q < 8; q += 2) kl = min(min(kl, lo[q]), lo[q + 1]), kh = min(min(kh, hi[q]), hi[q + 1]);
    const uint32_t km = min(kl, kh);
    if constexpr (FIRST) {
        best = MfmaBest{km, kl, (uint32_t)t};
    } else {
        const bool better = (km | ((1u << kMfmaKT) - 1u)) < best.k;
        best.k = better ? km : best.k;
        best.l = better ? kl : best.l;
        best.t = better ? (uint32_t)t : best.t;
    }
}

// a ring cursor: on by one row, back to the ring's first row behind its last
__device__ __forceinline__ void mfma_advance(uint32_t &at, uint32_t row, uint32_t end)
{
    at += row;
    at = at == end ? 0u : at;
}

template <int WW, int WH>
__global__ void __launch_bounds__(64 * kMfmaWaves) ws_march_mfma_kernel(const MarchArgs g)
{
    constexpr int NW = kMfmaWaves, NV = kMfmaVTiles, NVW = kMfmaTilesPerWave, KT = kMfmaKT, NT = 64 * NW, TX = 32 * kMfmaXWaves;
    constexpr int NR = mfma_ring_rows(WH);
    constexpr int K = 3 * WW;
    static_assert(K <= 32 && K > 16, "one row of the window is one K = 32 step, its pad in the upper lane half");
    static_assert(mfma_key_ranges_hold<K, WH>(), "the ranges of the packed key (above)");
    static_assert(KT == 3, "(Acc << (KT + 1)) + bias' is one v_lshl_add_u64 per register pair for a shift of 4");
    static_assert(kMfmaXWaves == 4 && kMfmaVWaves == 2, "wave >> 2 is the share of the tiles");

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

    // the raw rings start as zeros: bytes outside the image are never copied and stay zero, which every consumer reads
    // as the centred byte -128 for the row's whole life (the candidates that read them are poisoned, their keys stay
    // bounded because -128 is a byte like any other: the first static_assert above)
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

    // ---- the rows a step touches: ring offsets (bytes) and the byte phases of raw index 0, one scalar each --------
    // Set once with a modulo, then advanced by one row per step.  Strip row i sits in slot i mod NR of the raw rings
    // and in slot i mod NRO of the operand ring.
    const uint32_t cpBase = wave == 0 ? ringA : ringB, cpRB = wave == 0 ? RBA : RBB; // (the copying waves)
    const int ipx = -WH - g.wy0; // the output row of step s - 1 has its own pixels in strip row s + ipx
    uint32_t cCp, aIn, aOut, aPx, bSt, oWr, oIn, oOut, oSq, phIn, phOut, phPx, phSt;
    auto set_cursors = [&](int s) __attribute__((always_inline)) {
        auto slot = [](int i, int rows) __attribute__((always_inline)) { return (uint32_t)(((i % rows) + rows) % rows); };
        cCp = slot(s + 3, NR) * cpRB;
        aIn = slot(s, NR) * RBA, aOut = slot(s - WH, NR) * RBA, aPx = slot(s + ipx, NR) * RBA;
        bSt = slot(s + 1, NR) * RBB;
        oWr = slot(s + 1, NRO) * OPROW, oIn = slot(s, NRO) * OPROW, oOut = slot(s - WH, NRO) * OPROW, oSq = slot(s + 1 - WH, NRO) * OPROW;
        phIn = (phA0 + (uint32_t)s * stA) & 15u, phOut = (phA0 + (uint32_t)(s - WH) * stA) & 15u, phPx = (phA0 + (uint32_t)(s + ipx) * stA) & 15u;
        phSt = (phB0 + (uint32_t)(s + 1) * stB) & 15u;
    };
    auto advance = [&]() __attribute__((always_inline)) {
        mfma_advance(cCp, cpRB, (uint32_t)NR * cpRB);
        mfma_advance(aIn, RBA, (uint32_t)NR * RBA), mfma_advance(aOut, RBA, (uint32_t)NR * RBA), mfma_advance(aPx, RBA, (uint32_t)NR * RBA);
        mfma_advance(bSt, RBB, (uint32_t)NR * RBB);
        mfma_advance(oWr, OPROW, (uint32_t)NRO * OPROW), mfma_advance(oIn, OPROW, (uint32_t)NRO * OPROW);
        mfma_advance(oOut, OPROW, (uint32_t)NRO * OPROW), mfma_advance(oSq, OPROW, (uint32_t)NRO * OPROW);
        phIn = (phIn + stA) & 15u, phOut = (phOut + stA) & 15u, phPx = (phPx + stA) & 15u, phSt = (phSt + stB) & 15u;
    };

    const bool wave_on = tile_x0 + 32 * wx < g.ox1; // (a wave all of whose columns lie past the interior only helps with the operand pass)

    // pad mask of an operand part: bytes K .. 31 of the 32 a lane pair holds are outside the window (h = 1 holds bytes 16 .. 31)
    ws_i32x4 amask;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int first = 16 * h + 4 * j; // this dword's first byte
        const int keep = K - first;       // bytes of it inside the window
        amask[j] = keep >= 4 ? -1 : keep <= 0 ? 0 : (int)((1u << (8 * keep)) - 1u);
    }
    const uint32_t pA_lane = ringA + 3u * (uint32_t)(32 * wx + n) + 16u * (uint32_t)h; // byte of this lane's operand part in a raw A row
    const uint32_t px_lane = ringA + 3u * (uint32_t)(32 * wx + n - g.st.wx0);         // ... of its own pixel

    __syncthreads();

    // tile j of a wave with share v is candidate tile t = v NVW + j; its smallest e = d - d_lo is 32 (NV - 1 - t) - 31
    auto tiles_active = [&](int v) __attribute__((always_inline)) {
        uint32_t on = 0u;
        for (int j = 0; j < (v == 0 ? NVW : NV - NVW); ++j)
            if (32 * (NV - 1 - (v * NVW + j)) - 31 <= dspan) on |= 1u << j;
        return on;
    };

    // ---- a wave's march down the strip; WV: its share of the tiles, and with it its role -------------------------
    // ALL: every tile of the wave has a candidate inside [d_lo, d_hi] -- the usual case; its tile loop has no branch, so
    // the compiler overlaps the tiles' operand reads, MFMAs and keys.  A narrow range takes the march that skips tiles.
    // (One march or the other for the whole strip: a choice per step would meet in copies of every accumulator.)
    auto march = [&](auto role, auto all) __attribute__((always_inline)) {
        constexpr int WV = decltype(role)::value;
        constexpr bool ALL = decltype(all)::value;
        constexpr int NTL = WV == 0 ? NVW : NV - NVW; // tiles of this wave
        constexpr int NI = WV == 0 ? 1 : 2;           // blocks of 32 target centres it prepares per step
        static_assert(kMfmaXWaves * (1 + 2) == (TX + 32 * (NV - 1)) / 32, "the waves' blocks are the tile row's");
        const uint32_t opB_lane = opB + 1024u * (uint32_t)(wx + WV * NVW) + 16u * (uint32_t)lane; // this wave's operands in an operand row, tile j: + 1024 j

        // ---- the operand pass: block blk0 + k, lane pair (n, n + 32) = target centre vb0 + 32 (blk0 + k) + n --------
        // tag: register i of a tile holds row m = (i & 3) + 8 (i >> 2) + 4 h of it; smaller m = larger d = preferred.  The
        // tag is the pair index i >> 1 (which word of the pair won, the tile's two minimum chains tell); G0 and the
        // poison ride in it, above the tag bits
        const int blk0 = WV == 0 ? wx : kMfmaXWaves + 2 * wx;
        const uint32_t st_lane = ringB + 3u * (uint32_t)(32 * blk0 + n) + 16u * (uint32_t)h; // this lane's 16 bytes in a raw B row
        const uint32_t it_lane = opB + 1024u * (uint32_t)blk0 + 16u * (uint32_t)lane;         // ... in an operand row
        const uint32_t it_hi = it_lane + (h == 0 ? 8u : 0u); // where the entry's upper 8 bytes go (items_enter)
        // ---- the row's sums: chunk WV kMfmaXWaves + wx, lane i = pixel cp0 + i of the raw B row = target centre cp0 + i ----
        // The window of centre v is pixels v .. v + WW - 1 of the raw row, so its sums are a box over per-pixel sums: a
        // lane forms the sum of squares q of its pixel's 3 centred bytes and the sum r of its 3 raw bytes, packs them
        // as (q << kSumShift) + r and adds the words of the WW - 1 lanes above it, fetched by DPP inside the additions
        // (wave_shl:1, lane 63 reads 0).  Lanes 0 .. CW - 1 of a chunk then hold whole windows and own their centres.  The
        // last chunk starts early enough to stay inside the row, and the eighth wave runs it a second time: a centre with
        // two owners gets the same words from both (same bytes in, same arithmetic), as the two lanes of a pair wrote the
        // one bias word before.  Lanes CW .. 63 hold cut windows; the step has no branch, so they store too, into pad
        // nobody reads (below).
        constexpr int CW = 64 - (WW - 1), NVC = TX + 32 * (NV - 1), kSumShift = 13;
        static_assert(WW * 3 * 128 * 128 < (1 << (32 - kSumShift)) && WW * 3 * 255 < (1 << kSumShift), "both window sums fit their fields of the packed word");
        static_assert((NVC + CW - 1) / CW <= NW && NVC >= CW, "a chunk per wave covers the tile row's centres");
        const int chunk = WV * kMfmaXWaves + wx;
        const int cp0 = min(CW * chunk, NVC - CW);
        const int cv = min(cp0 + lane, NVC - 1); // (lanes past the last centre own nothing; their addresses stay inside the row)
        const bool c_own = lane < CW;
        uint32_t gsum = 0u, btag; // (window sum of b^^2) + 2 E, modulo 2^32; the tie tag, G0 and the poison
        {
            const int v = vb0 + cv, nn = cv & 31;
            const bool bvalid = (uint32_t)(v - g.st.b_lo) <= (uint32_t)(g.st.b_hi - g.st.b_lo) && g.st.b_hi >= g.st.b_lo;
            btag = (uint32_t)(((nn & 3) >> 1) + 2 * (nn >> 3)) + ((uint32_t)(kMfmaG0 + (bvalid ? 0 : kMfmaBiasPoison)) << KT);
        }
        const uint32_t cs_lane = ringB + 3u * (uint32_t)(cp0 + lane); // this lane's pixel in a raw B row
        // An operand entry has room for the window's sum of squares: in the h = 1 lane of a pair dwords 2 and 3 are bytes
        // 24 .. 31 of the centre's 32, which amask zeroes on the A side, so what the B side holds there is multiplied by
        // zero.  The centre's owner keeps the sum in dword 2 of that entry and reads it back when the row leaves.  The
        // wave that writes the entry is another one, in the same step: its h = 1 lanes store only the 8 bytes that
        // hold window bytes (items_enter), so the pad has one writer.  Dword 3 is read by nobody: the lanes that own
        // no centre store their words there, in any row of the ring.
        static_assert(K <= 24, "bytes 24 .. 31 of an operand entry are pad");
        const uint32_t pad_lane = opB + 1024u * (uint32_t)(cv >> 5) + 16u * (uint32_t)(32 + (cv & 31)) + 8u;
        const uint32_t sq_lane = pad_lane + (c_own ? 0u : 4u); // the entering row's sum is written there, the leaving row's read
        const uint32_t bi_lane = c_own ? biasr + 4u * (uint32_t)cv : pad_lane + 4u;
        const uint32_t bi_par = c_own ? 4u * (uint32_t)L.nvc : 0u;   // the bias rows are a double buffer

        // ---- the accumulators -----------------------------------------------------------------------------------
        // tile t, register i: e = d - d_lo = 32 (NV - 1 - t) + n - m; outside [0, dspan]: poisoned for good
        ws_i32x16 acc[NTL];
        const uint32_t active = tiles_active(WV); // this wave's tiles with a valid candidate
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            const int t = WV * NVW + j;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = (i & 3) + 8 * (i >> 2) + 4 * h;
                const int e = 32 * (NV - 1 - t) + n - m;
                acc[j][i] = (int)((uint32_t)e <= (uint32_t)dspan ? kMfmaA0 : kMfmaA0 + kMfmaAccPoison);
            }
        }

        MfmaRaw ir[NI];          // the entering row's raw bytes: the blocks' ...
        uint32_t cd0 = 0u, cd1 = 0u, csh = 0u; // ... and the chunk's pixel
        uint32_t il = 0u;        // the leaving row's window sum of squares, as it was stored when the row entered
        auto items_load = [&](auto leaves) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < NI; ++k) ir[k] = mfma_raw_load(st_lane + 96u * (uint32_t)k + bSt + phSt);
            const uint32_t at = cs_lane + bSt + phSt;
            const lds_u32 *q = lds_at32(at & ~3u);
            cd0 = q[0], cd1 = q[1], csh = at & 3u;
            if constexpr (decltype(leaves)::value) il = *lds_at32(sq_lane + oSq);
        };
        // what a pipelined step reads before the barrier of the step before it (issue order = order of use): the two
        // raw A rows, the leaving row's operands, the operand pass's rows.  None of it is written in that step: the A
        // rows were copied two and more steps earlier, the raw B row one step earlier, the leaving rows' operands WH - 1
        // and WH steps earlier.  (The entering row's operands, the bias' values and the merge pairs ARE written in it.)
        MfmaRaw n_rae{}, n_ral{};
        uint4 n_bl[NTL];
        auto ahead_load = [&]() __attribute__((always_inline)) {
            n_rae = mfma_raw_load(pA_lane + aIn + phIn);
            n_ral = mfma_raw_load(pA_lane + aOut + phOut);
#pragma unroll
            for (int t = 0; t < NTL; ++t) n_bl[t] = lds_load128(opB_lane + oOut + 1024u * (uint32_t)t);
            items_load(std::true_type());
        };
        // row iu enters the windows of the target centres, row iu - WH leaves them; in parts, so that the pipelined step
        // can place them under different MFMAs: the entering row's operands, block k ...
        auto items_enter = [&](int k) __attribute__((always_inline)) {
            // centred and masked in one v_bitop3 per dword, as the A operands are: the stored B operand has zeros in its
            // pad too (the A side multiplies the pad by zero either way)
            const ws_i32x4 cm = (mfma_raw_align(ir[k]) ^ (int)0x80808080u) & amask;
            // two stores of 8 bytes, the upper half first: the h = 0 lanes put it behind the lower half, the h = 1 lanes,
            // whose upper half is pad that belongs to the sums' owner, at the lower half's own address, where the second
            // store (a wave's LDS operations complete in order) overwrites it
            *reinterpret_cast<lds_i64 *>((uintptr_t)(it_hi + 1024u * (uint32_t)k + oWr)) = ws_i32x2{cm.z, cm.w};
            *reinterpret_cast<lds_i64 *>((uintptr_t)(it_lane + 1024u * (uint32_t)k + oWr)) = ws_i32x2{cm.x, cm.y};
        };
        // ... the chunk's packed window sums ...
        uint32_t cbox = 0u;
        auto sums_box = [&]() __attribute__((always_inline)) {
            const uint32_t x = __builtin_amdgcn_alignbyte(cd1, cd0, csh); // the pixel's 3 bytes and one of the next
            const int c = (int)((x ^ 0x80808080u) & 0x00ffffffu); // (the constant the operands are centred with)
            const uint32_t q = (uint32_t)__builtin_amdgcn_sdot4(c, c, 0, false);
            const uint32_t r = __builtin_amdgcn_udot4(x, 0x00010101u, 0u, false);
            const uint32_t w = (q << kSumShift) + r;
            uint32_t s = w;
            // (mov_dpp, not update_dpp(0, ...): see ws_march_kernel.h; the move folds into the addition)
#pragma unroll
            for (int j = 1; j < WW; ++j) s = w + (uint32_t)__builtin_amdgcn_mov_dpp((int)s, 0x130, 0xf, 0xf, true); // wave_shl:1
            cbox = s;
        };
        // ... and the leaving row's sum (read back, not computed again), the running total and the bias' value.  A ring
        // byte outside the image is the byte -128 like any other: r counts it as 0, and sum b^ = r - 128 K.
        auto sums_leave = [&](int iu, auto leaves) __attribute__((always_inline)) {
            const uint32_t q = cbox >> kSumShift, r = cbox & ((1u << kSumShift) - 1u);
            uint32_t u = q + 2u * r - 2u * 128u * (uint32_t)K;
            if constexpr (decltype(leaves)::value) u -= il;
            gsum += u;
            *reinterpret_cast<lds_u32 *>((uintptr_t)(sq_lane + oWr)) = q;
            *reinterpret_cast<lds_u32 *>((uintptr_t)(bi_lane + (uint32_t)(iu & 1) * bi_par)) = (gsum << KT) + btag;
        };
        auto items_finish = [&](int iu, auto leaves) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < NI; ++k) items_enter(k);
            sums_box();
            sums_leave(iu, leaves);
        };

        // ---- the output row of step sp: the better of the two waves' candidates, the fallback, the black-pixel rule ----
        int my_cw = 0, my_G = 0; // this wave's own best of the last step
        struct Flush {
            ws_i32x2 o;
            uint32_t q0, q1, sh;
        };
        auto flush_load = [&](int sp) __attribute__((always_inline)) {
            Flush f;
            f.o = *reinterpret_cast<const lds_i64 *>((uintptr_t)(mrg + 8u * (uint32_t)((sp & 1) * TX + 32 * wx + n)));
            // black pixel: the output pixel's own bytes, raw, in ring A
            const uint32_t p = px_lane + aPx + phPx;
            const lds_u32 *q = lds_at32(p & ~3u);
            f.q0 = q[0], f.q1 = q[1], f.sh = p & 3u;
            return f;
        };
        auto flush_store = [&](int sp, const Flush &f) __attribute__((always_inline)) {
            int cw = my_cw, G = my_G;
            if (f.o.x < cw || (f.o.x == cw && f.o.y < G)) { cw = f.o.x; G = f.o.y; }
            const int x = tile_x0 + 32 * wx + n, y = ys + sp - (WH - 1);
            if (h == 0 && x < g.ox1) {
                float val;
                if (cw >= (int)kMfmaValidBound) val = g.fallback_neg ? -(float)x : (float)x; // no valid candidate
                else val = (float)(g.d_lo + 32 * (NV - 1) + n - G);
                if ((__builtin_amdgcn_alignbyte(f.q1, f.q0, f.sh) & 0x00ffffffu) == 0u) val = 0.0f;
                if (g.out16) g.out16[(size_t)y * g.out_pitch + x] = (int16_t)(int)val;
                else g.out[(size_t)y * g.out_pitch + x] = val;
            }
        };

        auto step = [&](int s, auto phase) __attribute__((always_inline)) {
            // PHASE -1: the stages alone, 0: rows enter, 1: the strip's first output row, 2: a row enters, a row leaves
            // (the steady phase: every stage has its row), 3: the same with the strip's end in sight
            constexpr int PHASE = decltype(phase)::value;
            constexpr bool STEADY = PHASE == 2;
            constexpr bool PIPE = ALL && PHASE >= 2; // the pipelined tile loop; the march that skips tiles keeps the simple one
            using Leaves = std::integral_constant<bool, (PHASE >= 1)>; // row s + 1 - WH exists
            Flush fl{};
            if constexpr (WV == 1 && PHASE >= 2) {
                if (wave_on) fl = flush_load(s - 1);
            }
            // the copy of row s + 3 (wave 0: image A, wave 1: image B)
            if constexpr (WV == 0) {
                if (wave < 2 && (STEADY || s + 3 < nsteps)) raw_dma(cpBase + cCp, dmaMine, s + 3, lane);
            }
            // row s + 1 of the target image: the lane-linear MFMA operands of its blocks, so that the waves that multiply
            // a block -- up to 8, when the row enters and again when it leaves -- read one aligned ds_read_b128 each, and
            // the bias' values of step s + 1
            const bool stage = STEADY || (s + 1 >= 0 && s + 1 < nsteps);
            if constexpr (STEADY) {
                if (!(PIPE && wave_on)) items_load(Leaves()); // (a pipelined step's were read ahead: ahead_load)
            }
            // the matrix cores: row s enters every window, row s - WH leaves it; keys and the output row
            if (PHASE >= 0 && wave_on) {
                MfmaRaw rae{}, ral{};
                if constexpr (PIPE) {
                    rae = n_rae, ral = n_ral;
                } else {
                    rae = mfma_raw_load(pA_lane + aIn + phIn);
                    if constexpr (PHASE >= 2) ral = mfma_raw_load(pA_lane + aOut + phOut);
                }
                const uint32_t opBe = opB_lane + oIn, opBl = opB_lane + oOut;
                (void)opBl;
                if constexpr (!PIPE) {
                    if constexpr (STEADY) items_finish(s + 1, Leaves());
                    else if (stage) { items_load(Leaves()); items_finish(s + 1, Leaves()); }
                }
                // -a^ - 1 = a xor 0x7f, a^ = a xor 0x80; the pad must stay zero
                ws_i32x4 ae{}, al{};
                if constexpr (!PIPE) {
                    ae = (mfma_raw_align(rae) ^ (int)0x7f7f7f7fu) & amask;
                    if constexpr (PHASE >= 2) al = (mfma_raw_align(ral) ^ (int)0x80808080u) & amask;
                }
                MfmaBest best{UINT_MAX, UINT_MAX, 0u}; // "none": every key is below it
                const uint32_t brow = biasr + 4u * (uint32_t)((s & 1) * L.nvc + 32 * (wx + WV * NVW) + 4 * h);
                if constexpr (PIPE) {
                    // ---- the pipelined tile loop (see the header) -----------------------------------------------
                    // LDS operations return in issue order, so the compiler's waits on this sequence are counts
                    uint4 be4[NTL], bq[2][4];
#pragma unroll
                    for (int t = 0; t < NTL; ++t) be4[t] = lds_load128(opBe + 1024u * (uint32_t)t);
#pragma unroll
                    for (int q = 0; q < 4; ++q) bq[0][q] = lds_load128(brow + 4u * (uint32_t)(8 * q));
                    __builtin_amdgcn_sched_barrier(0); // every read above is in flight before the first wait
                    // Four groups of MFMAs with the operand pass's VALU between them.  Inside a group the compiler
                    // may take the MFMAs in any order, so the groups are cut where no order puts two MFMAs on one
                    // accumulator side by side: entering tiles 0 .. NTL - 3 | NTL - 2, NTL - 1 | leaving 0, 1 | 2 .. NTL - 1
                    auto enter = [&](int t) __attribute__((always_inline)) {
                        const ws_i32x4 be = {(int)be4[t].x, (int)be4[t].y, (int)be4[t].z, (int)be4[t].w};
                        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(be, ae, acc[t], 0, 0, 0);
                    };
                    auto leave = [&](int t) __attribute__((always_inline)) {
                        const ws_i32x4 bl = {(int)n_bl[t].x, (int)n_bl[t].y, (int)n_bl[t].z, (int)n_bl[t].w};
                        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bl, al, acc[t], 0, 0, 0);
                    };
                    constexpr int VG = kPipeValu[WV];
                    ae = (mfma_raw_align(rae) ^ (int)0x7f7f7f7fu) & amask;
                    al = (mfma_raw_align(ral) ^ (int)0x80808080u) & amask;
#pragma unroll
                    for (int t = 0; t < NTL - 2; ++t) enter(t);
                    if constexpr (STEADY) items_enter(0);
                    __builtin_amdgcn_sched_group_barrier(0x2, kPipeValuA, 0); // (the entering row's A operand)
#pragma unroll
                    for (int t = 0; t < NTL - 2; ++t) {
                        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x2, VG, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    enter(NTL - 2), enter(NTL - 1);
                    if constexpr (STEADY) {
                        if constexpr (NI == 2) items_enter(1);
                        else sums_box();
                    }
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x2, VG, 0);
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x2, VG, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!STEADY) {
                        if (stage) { items_load(Leaves()); items_finish(s + 1, Leaves()); }
                    }
                    leave(0), leave(1);
                    if constexpr (STEADY) {
                        if constexpr (NI == 2) sums_box();
                        else sums_leave(s + 1, Leaves());
                    }
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x2, VG, 0);
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x2, VG, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (STEADY && NI == 2) {
                        sums_leave(s + 1, Leaves());
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    advance(); // (nothing below names a cursor of this step)
#pragma unroll
                    for (int t = 0; t < NTL; ++t) {
                        // the next step's reads, two tiles' keys ahead of the barrier; the next tile's bias quads (they
                        // have a tile's keys to land in) and the leaving MFMA of the tile after it, then this tile's keys
                        // under that MFMA
                        if (t == NTL - 2) ahead_load();
                        if (t + 1 < NTL) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) bq[(t + 1) & 1][q] = lds_load128(brow + 4u * (uint32_t)(32 * (t + 1) + 8 * q));
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (t + 2 < NTL) {
                            leave(t + 2);
                            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                        }
                        if (t == 0) mfma_tile_best<true>(acc[t], bq[t & 1], t, best);
                        else mfma_tile_best<false>(acc[t], bq[t & 1], t, best);
                    }
                } else
#pragma unroll
                for (int t = 0; t < NTL; ++t) { // (t: the tile's index in this wave)
                    if constexpr (!ALL) {
                        if (!(active & (1u << t))) continue; // (uniform)
                    }
                    const uint4 be4 = lds_load128(opBe + 1024u * (uint32_t)t);
                    const ws_i32x4 be = {(int)be4.x, (int)be4.y, (int)be4.z, (int)be4.w};
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(be, ae, acc[t], 0, 0, 0);
                    if constexpr (PHASE >= 2) {
                        const uint4 bl4 = lds_load128(opBl + 1024u * (uint32_t)t);
                        const ws_i32x4 bl = {(int)bl4.x, (int)bl4.y, (int)bl4.z, (int)bl4.w};
                        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bl, al, acc[t], 0, 0, 0);
                    }
                    if constexpr (PHASE >= 1) {
                        uint4 b4[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) b4[q] = lds_load128(brow + 4u * (uint32_t)(32 * t + 8 * q));
                        if (ALL && t == 0) mfma_tile_best<true>(acc[t], b4, t, best);
                        else mfma_tile_best<false>(acc[t], b4, t, best);
                    }
                }
                if constexpr (PHASE >= 1) {
                    // the two halves of a column: G = 32 t + m orders ALL its candidates (smaller = larger d)
                    const uint32_t bestc = mfma_best_code(best); // 2 t + (the high word of the pair won)
                    const int i_best = 2 * (int)(best.k & ((1u << KT) - 1u)) + (int)(bestc & 1u);
                    int G = 32 * ((int)(bestc >> 1) + WV * NVW) + (i_best & 3) + 8 * (i_best >> 2) + 4 * h;
                    int cw = (int)(best.k >> KT); // the cost word (+ kMfmaC0): below 2^29
                    mfma_pair_best(cw, G);
                    if constexpr (WV == 1 && PHASE >= 2) flush_store(s - 1, fl);
                    // the first wave of a column leaves its best in LDS for the second, which writes the row out in the
                    // next step (both lanes of a column write the one pair)
                    if constexpr (WV == 0) {
                        *reinterpret_cast<lds_i64 *>((uintptr_t)(mrg + 8u * (uint32_t)((s & 1) * TX + 32 * wx + n))) = ws_i32x2{cw, G};
                    } else {
                        my_cw = cw;
                        my_G = G;
                    }
                }
            } else {
                if constexpr (STEADY) items_finish(s + 1, Leaves());
                else if (stage) { items_load(Leaves()); items_finish(s + 1, Leaves()); }
            }
            if constexpr (WV == 0) {
                if (wave < 2) dma_wait(); // (the copy lands inside its step: a wait that lets it span the barrier measured slower)
            }
            __syncthreads();
            if constexpr (PIPE) {
                if (!wave_on) advance(); // (a wave with columns advanced in the middle of its step)
            } else {
                advance();
                // the first pipelined step's reads
                if constexpr (ALL && PHASE == 1) {
                    if (wave_on) ahead_load();
                }
            }
        };

        int s = -3;
        set_cursors(s);
#pragma unroll 1
        for (; s < 0; ++s) step(s, std::integral_constant<int, -1>());
#pragma unroll 1
        for (; s < WH - 1; ++s) step(s, std::integral_constant<int, 0>());
        step(s++, std::integral_constant<int, 1>());
#pragma unroll 1
        for (; s + 3 < nsteps; ++s) step(s, std::integral_constant<int, 2>());
#pragma unroll 1
        for (; s < nsteps; ++s) step(s, std::integral_constant<int, 3>());
        if constexpr (WV == 1) {
            if (wave_on) flush_store(nsteps - 1, flush_load(nsteps - 1)); // the last row
        }
    };
    const bool all = tiles_active(wv) == (1u << (wv == 0 ? NVW : NV - NVW)) - 1u;
    if (wv == 0) {
        if (all) march(std::integral_constant<int, 0>(), std::true_type());
        else march(std::integral_constant<int, 0>(), std::false_type());
    } else {
        if (all) march(std::integral_constant<int, 1>(), std::true_type());
        else march(std::integral_constant<int, 1>(), std::false_type());
    }
}

} // namespace wsamd
