// ws_search.h -- the search dispatch (ws_search.cpp).  Knows ws_params and ws_image, not ws_context: a search reads and
// leaves nothing but its arguments and the Searcher, which owns what only the search touches (the context holds one).
#pragma once

#include "ws_capi_internal.h"
#include "ws_kernels.h"

#pragma GCC visibility push(hidden)
namespace wsamd {

struct Searcher {
    int num_cus = 256; // the device's, for the planner
    DevBuf plane_a, plane_b, keys, cost, bs_plane, max_block, sel, sel_planes, top3;
    DevBuf ct_left, ct_right; // a census cost: the descriptor planes of both images (ws_ct.h)
    // the last few problems' plans, keyed on (Canon, tuning): a queue of equal pairs asks for the same one every call, the
    // left-right check for two in turn, and the planner walks every strip count for two thread shapes, up to three
    // candidate tilings and two workgroup sizes -- 5 us of a 15 us enqueue
    struct CachedPlan {
        bool valid = false, ok = false; // ok: march_plan's answer (launch holds a plan)
        Canon canon{};
        int tune[3] = {0, 0, 0};
        MarchLaunch launch{};
    };
    CachedPlan plans[4];
    int plan_next = 0; // the entry the next new problem replaces (round robin)
    const CachedPlan &plan_for(const Canon &c);
    int tune[3] = {0, 0, 0};              // ws_set_tuning: x-runs per tile, strip rows, threads (0 = automatic)
    ScratchLease lease;                   // every search holds it: the scratch planes above are shared across streams
    bool profiling = false, kernel_timed = false; // ws_set_profiling; evk0 / evk1 bracket the last marching kernel
    hipEvent_t evk0 = nullptr, evk1 = nullptr;
    std::string last_kernel; // ws_last_launch_info
    int last_threads = 0, last_wgs = 0, last_lds = 0;
    void launched(const char *kernel, int threads, int wgs, int lds) { last_kernel = kernel; last_threads = threads; last_wgs = wgs; last_lds = lds; }
    bool var_block_ran = false; // the last right-view search grew windows: max_block holds the largest (ws_last_max_block)
};

inline bool image_ok(const ws_image *im) { return im && im->data && im->width > 0 && im->height > 0 && im->stride >= 3 * im->width; }
// The checks every search entry point makes (err == nullptr: the message goes to ws_last_error(NULL)).
int check_params(std::string *err, const ws_params *p, const ws_image *L, const ws_image *R);
// A host call's map buffer for the search p on L, R (or on their rectified forms): its pointer and type, and rows of at
// least the map's width.  The map's size goes to *ow x *oh.
int check_out(std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, const void *out, int out_stride,
              int out_dtype, int *ow, int *oh);
// Reduce LEFT / RIGHT to the canonical search.  Returns false when no marching region exists.
bool make_canon(const ws_params *p, const ws_image *L, const ws_image *R, Canon *c);
int wire_for(const ws_params *p, const ws_image *L, const ws_image *R);

// One search on device images, on stream s: the map to `out` (out_stride floats per row), or as 16-bit integers to `out16`
// (same pitch; only if wire_for is kWireI16).  status: the mapped words the kernels flag trouble in.
int search(Searcher &S, std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, float *out,
           int out_stride, int16_t *out16, unsigned int *status, hipStream_t s);

} // namespace wsamd
#pragma GCC visibility pop
