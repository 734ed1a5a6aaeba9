// ws_ct.h -- the census-transform matching cost on the device (ws_ct.hip), for ws_search.cpp, ws_sgm.cpp / ws_sgm.hip and
// ws_capi.cpp.  Internal; the rules are in include/ws_stereo.h ("census-transform matching cost").
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#pragma GCC visibility push(hidden)
namespace wsamd {

constexpr int kCtThreads = 256;
constexpr int kCtTile = 64;   // match kernel: columns per workgroup (16 per wave)
constexpr int kCtStrip = 32;  // match kernel: rows per workgroup
constexpr int kCtMaxHalf = 31; // block_size <= 63
constexpr int kCtCols = kCtTile + 2 * kCtMaxHalf;
constexpr int kCtWtaStep = 62; // winner-take-all sink: candidates a 64-lane chunk owns (lanes 0 and 63 are the parabola's neighbours)
// static LDS of the match kernel: the column sums (16 bits each), and for the winner-take-all sink four words per pixel
constexpr int kCtLdsVolume = kCtCols * 64 * 2;
constexpr int kCtLdsWta = kCtLdsVolume + 4 * 4 * kCtStrip * kCtTile;
constexpr const char *kCtMatchKernel = "ws_census_match_kernel";

inline bool is_census(int cost) { return cost == WS_COST_CENSUS_5X5 || cost == WS_COST_CENSUS_9X7; }
inline int census_bits(int cost) { return cost == WS_COST_CENSUS_5X5 ? 24 : 62; }
// bytes of one descriptor in a plane of the searches (the public transform always widens to 8)
inline size_t census_plane_elem(int cost) { return cost == WS_COST_CENSUS_5X5 ? 4 : 8; }

// One match: the window sums of popcount(T_L xor T_R) over the disparities d = d0 + j, j < nd, for every pixel of the
// view's map (w x h), into one of two sinks.
struct CtMatchArgs {
    const void *TL, *TR;  // descriptor planes, dense: w1 x h1 and w2 x h2 (uint32 for 5x5, uint64 for 9x7)
    const uint8_t *L, *R; // the BGR images: the view's black test
    int w1, h1, s1, w2, h2, s2;
    int wide;   // 64-bit descriptors
    int right;  // 0: left view, 1: right view
    int half;   // (block_size - 1) / 2
    int d0, nd; // d = d0 + j for j < nd (nd already clipped to what the geometry allows)
    int w, h;   // the map
    int subpixel;
    float *out; // sink (a): the map
    int out_pitch;
    void *cost; // sink (b): C(p, j), w*h*nd of uint16 (cost16) or uint32, j innermost (SgmArgs::cost)
    int cost16;
};

// The disparities a search looks at: what the geometry allows of the view's range (every pixel's candidates lie inside).
// Left view d = 1 .. min(maxD, w1 - 1 - 2 half); right view d = minD .. min(maxD, w1) - 1.
inline void disparity_range(const ws_params *p, const ws_image *L, int *d0, int *nd)
{
    const int half = (p->block_size - 1) / 2;
    if (p->view == WS_VIEW_LEFT) {
        *d0 = 1;
        *nd = std::max(0, std::min(p->max_disparity, L->width - 1 - 2 * half));
    } else {
        *d0 = p->min_disparity;
        *nd = p->max_disparity <= p->min_disparity ? 0 : std::max(0, std::min(p->max_disparity, L->width) - p->min_disparity);
    }
}

// The geometry of a match (everything but the sinks).
inline CtMatchArgs census_match_args(const ws_params *p, const ws_image *L, const ws_image *R, const void *TL, const void *TR)
{
    CtMatchArgs a{};
    a.TL = TL; a.TR = TR;
    a.L = L->data; a.R = R->data;
    a.w1 = L->width; a.h1 = L->height; a.s1 = L->stride;
    a.w2 = R->width; a.h2 = R->height; a.s2 = R->stride;
    a.wide = p->cost == WS_COST_CENSUS_9X7;
    a.right = p->view == WS_VIEW_RIGHT;
    a.half = (p->block_size - 1) / 2;
    disparity_range(p, L, &a.d0, &a.nd);
    a.w = a.right ? R->width : L->width;
    a.h = a.right ? R->height : L->height;
    a.subpixel = p->subpixel != 0;
    return a;
}

inline long long census_match_workgroups(int w, int h) { return (long long)((w + kCtTile - 1) / kCtTile) * ((h + kCtStrip - 1) / kCtStrip); }

// The descriptors of a whole image: out_pitch elements per row, of 8 bytes (widen, or 9x7) or 4 (5x5 planes of the searches).
hipError_t launch_census_transform(const uint8_t *img, int w, int h, int stride, int cost, void *out, int out_pitch, bool widen,
                                   hipStream_t s);
// volume: sink (b), else sink (a).
hipError_t launch_census_match(const CtMatchArgs &a, bool volume, hipStream_t s);

} // namespace wsamd
#pragma GCC visibility pop
