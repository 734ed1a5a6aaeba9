// ws_sgm.h -- semi-global matching on the device (ws_sgm.hip), for ws_sgm.cpp.  Internal; the rules are in
// include/ws_stereo.h.
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

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
hipError_t launch_sgm(const SgmArgs &a, int paths, hipStream_t s);
// The same volumes, then the winner with the uniqueness test.  paths == 0: the block route -- no path kernel runs and the
// winner reads C (a.sum is not touched).
hipError_t launch_unique(const SgmArgs &a, const UniqueArgs &u, int paths, hipStream_t s);

} // namespace wsamd
#pragma GCC visibility pop
