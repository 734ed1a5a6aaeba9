// ws_sgm.h -- semi-global matching on the device (ws_sgm.hip), for ws_sgm.cpp.  Internal; the rules are in
// include/ws_stereo.h.
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#pragma GCC visibility push(hidden)
namespace wsamd {

constexpr int kSgmMaxNd = 2048; // disparities a path wave keeps in registers (32 per lane)

// One SGM search.  Disparity index j = 0 .. nd-1 stands for d = d0 + j.  The output map is w x h (the left image for
// the left view, the right image for the right view); every per-pixel plane below is dense, w x h.
struct SgmArgs {
    const uint8_t *L, *R;
    int w1, h1, s1, w2, h2, s2;
    int right;  // 0: left view, 1: right view
    int ssd;
    const void *TL, *TR; // a census cost: the descriptor planes of both images (ws_ct.h), else null
    int census_wide;     // ... of 64 bits (9x7) or 32 (5x5)
    int half;   // (block_size - 1) / 2
    int d0, nd; // d = d0 + j for j < nd (nd already clipped to what the geometry allows)
    int w, h;   // the map
    uint32_t p1, p2;
    uint32_t *kr;   // per pixel: node: lo | hi << 16 (hi > lo); no candidate: 0xffffffff; else 0
    void *cost;     // C(p, j): w*h*nd of uint16 (cost16) or uint32, j innermost
    void *sum;      // S(p, j): w*h*nd of uint32 (sum64 == 0) or uint64
    int cost16, sum64;
    int subpixel;
    float *out;
    int out_pitch;
};

// The uniqueness test and the confidence plane of one winner pass (ws_unique_wta_kernel).
struct UniqueArgs {
    int ratio;                  // 0 .. 100
    float *conf;                // the confidence plane, or null
    int conf_pitch;
    unsigned long long *counts; // {failed nodes, nodes}: zero on entry, one atomic add per wave and word
    int num_cus;
};

// The largest window cost of a search with cost WS_COST_* (a square window of bs x bs pixels: three channels, or the bits
// of a census descriptor).
inline uint64_t sgm_cost_max(int cost, int block_size)
{
    const uint64_t px = cost == WS_COST_SSD ? 3ull * 65025ull : cost == WS_COST_SAD ? 3ull * 255ull : cost == WS_COST_CENSUS_5X5 ? 24ull : 62ull;
    return px * (uint64_t)block_size * block_size;
}

// The cost plane (a census cost: from the match kernel of ws_ct.hip), the paths (`paths` 4 or 8, one launch each, summed in place in order on s) and the winner.
// paths == 0 (the pair call's block route): no path kernel runs and the winner reads C.
hipError_t launch_sgm(const SgmArgs &a, int paths, hipStream_t s);
// The same volumes, then the winner with the uniqueness test.  paths == 0: the block route -- no path kernel runs and the
// winner reads C (a.sum is not touched).
hipError_t launch_unique(const SgmArgs &a, const UniqueArgs &u, int paths, hipStream_t s);

// The pair call's derived map (ws_pair_wta_kernel): a row of the derived map keeps one 64-bit slot per column in LDS.
// Rows wider than kPairSwitchWidth are cut into spans of kPairSpan derived columns, each reading the kPairSpan + nd - 1
// base columns that reach it; 4 KiB of LDS per workgroup lets eight workgroups share a compute unit.  The switch is
// the span itself: a row of at most kPairSpan columns is one span.
constexpr int kPairSpan = 512;
constexpr int kPairSwitchWidth = kPairSpan;
// The derived map wd x hd into out, from the volume a launch_sgm / launch_unique with the same a and paths left behind on
// s (paths == 0: from C).  a.out is not touched.
hipError_t launch_pair_wta(const SgmArgs &a, int paths, float *out, int out_pitch, int wd, int hd, hipStream_t s);

// ---- host side, shared by ws_sgm.cpp and ws_pair.cpp ----
// The argument checks of the SGM calls.  sgm_optional: the uniqueness and pair calls, where a null sgm is the block
// route and only a given one is checked.
int check_sgm(std::string *err, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R,
              bool sgm_optional = false);
int check_ratio(std::string *err, const ws_unique_params *uq); // a given ws_unique_params
// The scratch of the call grown to what it needs, a census cost's descriptor planes on s, and the kernels' arguments
// for the map `out`.  Under the context's SGM lease.
int sgm_prepare(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R, float *out,
                int out_stride, hipStream_t s, SgmArgs *args);
// The volumes and the winner of `a` on s: the uniqueness winner with uq (its counts on their way to the host, the
// confidence plane conf or null), else the plain one.
int sgm_winner(ws_context *ctx, const SgmArgs &a, const ws_sgm_params *sgm, const ws_unique_params *uq, float *conf, int conf_stride,
               hipStream_t s);

} // namespace wsamd
#pragma GCC visibility pop
