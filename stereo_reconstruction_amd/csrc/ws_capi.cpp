// ws_capi.cpp -- the C-ABI of include/ws_stereo.h: argument checks that stand in for the
// reference's cv::Exception paths, reduction of the three reference methods to the canonical
// search (ws_kernels.h), scratch memory owned by the context, and the entry points that move the
// caller's host buffers (through ws_staging.h).  Compiled with hipcc; no compute happens on the host.
// The Middlebury plumbing (PFM, calib.txt, evaldisp) is in ws_io.cpp.
#include "../../include/ws_stereo.h"
#include "ws_kernels.h"
#include "ws_rectify.h"
#include "ws_capi_internal.h"
#include "ws_staging.h"

#include <errno.h>
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <string>
#include <vector>

using namespace wsamd;

namespace {

// device memory of the context (ensure), freed with its owner: ws_destroy makes the context's device current and its
// streams idle before it deletes the context
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct Job { // one pair in flight on the batched host path
    DevBuf in;               // left image, then right image (rows with the caller's stride, or gathered dense)
    DevBuf out, out16;       // the map as float32 / int16
    int wire = 0;            // the wire format this pair's map comes down in
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
    void *user_out = nullptr;
    int w = 0, h = 0, out_stride = 0, dtype = 0;
    int row0 = 0;         // the first row of the device map that goes to user_out (a row band: its halo rows stay behind)
    bool pending = false; // searched (or being searched), result not yet on its way to user_out
    HostBuf h_left, h_right; // stages of the images, or their gathered rows (image_span)
    HostBuf h_out;           // stage of a pageable map (HostSpan)
    int out_span = -1;       // index of this pair's output span in ws_context::batch_spans
};

thread_local std::string g_create_error; // ws_last_error(NULL): why the last ws_create on this thread failed

// development knob WS_HOST_TRACE=1: where the host's time goes inside a boundary call (stderr, microseconds since the call began)
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    std::string line;
    HostTrace() : on([] { static const bool v = [] { const char *e = getenv("WS_HOST_TRACE"); return e && atoi(e) == 1; }(); return v; }()), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what, int k = -1)
    {
        if (!on) return;
        char buf[64];
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (k >= 0) snprintf(buf, sizeof buf, " %s%d=%.0f", what, k, us); else snprintf(buf, sizeof buf, " %s=%.0f", what, us);
        line += buf;
    }
    ~HostTrace() { if (on && !line.empty()) fprintf(stderr, "[ws host trace, us]%s\n", line.c_str()); }
};

} // namespace

struct ws_context {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evk0 = nullptr, evk1 = nullptr;
    hipEvent_t ev_scratch = nullptr;      // end of the last search: the scratch planes are free again
    hipStream_t scratch_stream = nullptr; // ... the stream it ran on
    bool scratch_busy = false;
    bool profiling = false, kernel_timed = false;
    DevBuf plane_a, plane_b, keys, cost, bs_plane, max_block, sel, sel_planes, top3, d_left, d_right, d_out, d_out64 /* the consumers' scratch */, d_out16;
    DevBuf d_rect_left, d_rect_right; // ws_search_unrectified_host: the rectified images
    DevBuf d_mesh, d_mesh_text;       // the mesh text (ws_mesh.hip): per-workgroup sums / offsets and the file's bytes
    HostBuf h_mesh[2];                // ... which come down through these two pinned chunks (kMeshChunk each)
    hipEvent_t ev_mesh[2] = {};       // a chunk has landed in h_mesh[i]
    Job jobs[2];             // ws_enqueue_host alternates between two slots
    int job_next = 0;
    hipStream_t copy_stream = nullptr; // host <-> device copies of the batched path, beside the searches
    hipStream_t down_stream = nullptr; // ws_search_host in bands: maps go down here while images still come up on copy_stream
    static constexpr int kMaxBands = 8;
    hipEvent_t ev_band_up[kMaxBands] = {}, ev_band_done[kMaxBands] = {}, ev_band_down[kMaxBands] = {};
    HostBuf status_page;               // 64 mapped pinned bytes: the words below
    unsigned int *status_host = nullptr, *status_dev = nullptr; // mapped pinned words the kernels flag trouble in (word 0: ws_smooth_left_bands_kernel gave up; word 1: the integer box filter met a value it cannot carry)
    DevBuf d_flag;                     // 256 bytes: word 0 = the integer box filter met a value it cannot carry
    bool plan_valid = false, plan_ok = false; // run_search: the last problem's plan
    Canon plan_canon{};
    int plan_tune[3] = {0, 0, 0};
    MarchLaunch plan_launch{};
    int last_outliers_path = 0;        // ws_last_outliers_path
    int last_how[3] = {0, 0, 0};       // ws_last_host_paths: how the last host call's left / right / out bytes crossed
    int last_wire = 0;                 // ... and the wire format of its map (ws_last_wire_format)
    std::vector<HostSpan> batch_spans; // caller buffers of the pairs enqueued since the last ws_wait (released there)
    HostBuf h_left, h_right, h_out;    // ws_search_host: stages (HostSpan), or gathered rows of cut-out images (image_span)
    HostBuf h_aux[2];                  // stages of the consumers' further buffers
    int host_bands = -1;               // ws_set_host_bands: 0 = never split, -1 = automatic
    std::string err;
    std::string last_kernel;
    int last_threads = 0, last_wgs = 0, last_lds = 0;
    bool var_block_ran = false;
    // what the last run_search left behind, for the passes that follow it (smoothFactor)
    bool last_march = false;
    Canon last_canon{};
    Plane last_pa{}, last_pb{};
    int last_skip[4] = {0, 0, 0, 0};
    bool want_cost = false;       // run_search: also leave the winners' costs (right view, smoothFactor)
    bool want_planes = false;     // run_search: also pack the dword planes (the left view's smoothFactor pass reads them)
    bool last_planes = false;     // ... and whether the last search did
    int32_t *last_cost = nullptr; // where it left them (pitch = plane width), or null
    int16_t *direct_i16 = nullptr; // run_search: the kernels store the map as 16-bit integers here (the wire format of a host call)
    int tune_nxr = 0, tune_rows = 0, tune_threads = 0;
};

namespace {

int fail(ws_context *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define WS_HIP(ctx, call)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, WS_ERR_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_),        \
                        __FILE__, __LINE__);                                                    \
    } while (0)

int ensure(ws_context *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return WS_OK;
    if (b.p) WS_HIP(ctx, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    WS_HIP(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return WS_OK;
}

bool image_ok(const ws_image *im)
{
    return im && im->data && im->width > 0 && im->height > 0 && im->stride >= 3 * im->width;
}

int check_params(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R)
{
    if (!p || !image_ok(L) || !image_ok(R)) return fail(ctx, WS_ERR_ARG, "null or malformed image / params");
    if (p->view != WS_VIEW_LEFT && p->view != WS_VIEW_RIGHT && p->view != WS_VIEW_LINEAR)
        return fail(ctx, WS_ERR_ARG, "unknown view %d", p->view);
    if (p->cost != WS_COST_SSD && p->cost != WS_COST_SAD) return fail(ctx, WS_ERR_ARG, "unknown cost %d", p->cost);
    if (p->view != WS_VIEW_LINEAR && (p->block_size < 1 || p->block_size > 63))
        return fail(ctx, WS_ERR_ARG, "blockSize %d outside [1,63]", p->block_size);
    if (p->view == WS_VIEW_LINEAR && p->linear_range < 1) return fail(ctx, WS_ERR_ARG, "linear_range < 1");
    if (!(p->smooth_factor == p->smooth_factor)) return fail(ctx, WS_ERR_ARG, "smoothFactor is NaN");
    if (p->var_block && p->view == WS_VIEW_RIGHT && p->subpixel)
        return fail(ctx, WS_ERR_UNSUPPORTED, "sub-pixel refinement together with varBlock");
    if (p->var_block && p->view == WS_VIEW_RIGHT && !(p->thres == p->thres))
        return fail(ctx, WS_ERR_ARG, "thres is NaN");
    if (p->subpixel && p->view == WS_VIEW_LINEAR) return fail(ctx, WS_ERR_UNSUPPORTED, "sub-pixel on LinearSearch");
    if (p->subpixel && p->smooth_factor != 1.0) return fail(ctx, WS_ERR_UNSUPPORTED, "sub-pixel refinement together with smoothFactor != 1");
    const int h1 = L->height, w1 = L->width, h2 = R->height;
    const int height = std::min(h1, h2);
    const int half = (p->block_size - 1) / 2;
    if (p->view == WS_VIEW_LEFT) {
        // Rect(x-half, y-half, bs, bs) leaves the image for even bs (BlockSearch.cpp:46-49)
        if ((p->block_size & 1) == 0 && height - 2 * half > 0 && w1 - 2 * half > 0)
            return fail(ctx, WS_ERR_GEOMETRY, "even blockSize %d: the reference throws cv::Exception", p->block_size);
    } else if (p->view == WS_VIEW_RIGHT && p->max_disparity > p->min_disparity) {
        if (p->min_disparity < 0)
            return fail(ctx, WS_ERR_GEOMETRY, "minDisparity < 0: left ROI starts before column 0 (BlockSearch.cpp:151)");
        // leftImage_(Rect(.., y-up, .., up+down)) needs y + down <= h1 (BlockSearch.cpp:151-154)
        for (int y = std::max(0, height - half - 1); y < height; ++y) { // (only the last rows can overrun)
            const int down = std::min(h2 - y - 1, half);
            if (y + down > h1)
                return fail(ctx, WS_ERR_GEOMETRY, "left image too short for the right view window at row %d", y);
        }
        // varBlock grows windows by data: with a right image taller than the left one a grown window near
        // row h1 needs left-image rows >= h1 and the reference throws (BlockSearch.cpp:151-154) -- but only
        // if such a pixel happens to grow.  Defined here: rejected up front, whatever the data.
        if (p->var_block && h2 > h1)
            return fail(ctx, WS_ERR_GEOMETRY, "varBlock with a right image taller than the left one: a grown window "
                                              "would leave the left image (BlockSearch.cpp:151-154)");
    }
    return WS_OK;
}

// Reduce LEFT / RIGHT to the canonical search.  Returns false when no marching region exists.
bool make_canon(const ws_params *p, const ws_image *L, const ws_image *R, Canon *c)
{
    const int h1 = L->height, w1 = L->width, h2 = R->height, w2 = R->width;
    const int height = std::min(h1, h2);
    const int half = (p->block_size - 1) / 2;
    Canon k{};
    k.ssd = p->cost == WS_COST_SSD;
    if (p->view == WS_VIEW_LEFT) {
        k.wa = w1; k.ha = h1; k.wb = w2; k.hb = h2;
        k.ww = k.wh = p->block_size;
        k.wx0 = k.wy0 = -half;
        k.boff = 0;
        // no candidate beyond what the geometry allows (x - d >= half with x <= w1 - 1 - half): a range far
        // wider than the image costs neither d-group passes nor tie-tag bits; the tags keep their order
        k.d_lo = 1; k.d_hi = k.d_hi_clipped = std::min(p->max_disparity, w1 - 1 - 2 * half);
        k.b_lo = half; k.b_hi = w2 - half - 1;
        k.ox0 = half; k.ox1 = w1 - half;
        k.oy0 = half; k.oy1 = height - half;
        k.prefer_large = 1; k.mirror = 0; k.fallback_neg = 0;
    } else if (p->view == WS_VIEW_RIGHT) {
        if (half < 1) return false;
        k.wa = w2; k.ha = h2; k.wb = w1; k.hb = h1;
        k.ww = k.wh = 2 * half;
        k.wx0 = 1 - half; k.wy0 = -half;
        k.boff = w1 - w2;
        // (x + d + half < w1 with x >= half: the same clamp)
        k.d_lo = p->min_disparity; k.d_hi = std::min(p->max_disparity - 1, w1 - 1 - 2 * half);
        k.d_hi_clipped = std::min(p->max_disparity - 1, w1 - 1); // border ring: x >= 0 and right >= 0 only
        k.b_lo = half; k.b_hi = w1 - 1 - half;
        k.ox0 = half; k.ox1 = w2 - half;
        k.oy0 = half; k.oy1 = std::min(h2 - half, height);
        k.prefer_large = 0; k.mirror = 1; k.fallback_neg = 1;
    } else {
        return false;
    }
    *c = k;
    return k.ox1 > k.ox0 && k.oy1 > k.oy0 && k.d_hi >= k.d_lo;
}

// the brute-force kernels' view of a search (ws_kernels.h)
GenericArgs generic_args(const ws_params *p, const ws_image *L, const ws_image *R, float *out, int out_stride)
{
    GenericArgs ga{};
    ga.L = L->data; ga.R = R->data;
    ga.w1 = L->width; ga.h1 = L->height; ga.s1 = L->stride;
    ga.w2 = R->width; ga.h2 = R->height; ga.s2 = R->stride;
    ga.view = p->view; ga.ssd = p->cost == WS_COST_SSD;
    ga.block_size = p->block_size; ga.min_d = p->min_disparity; ga.max_d = p->max_disparity;
    ga.linear_range = p->linear_range;
    ga.out = out; ga.out_pitch = out_stride;
    return ga;
}

int run_search(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R,
               float *out, int out_stride, hipStream_t s);

int run_device_on(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R,
                  float *out, int out_stride, hipStream_t s);

// The context's scratch planes are shared by every call: a call on another stream than the previous
// one first waits (on the device) for that previous call to be done with them.
int run_device(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R,
               float *out, int out_stride, hipStream_t s)
{
    if (ctx->scratch_busy && s != ctx->scratch_stream) WS_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_scratch, 0));
    const int rc = run_device_on(ctx, p, L, R, out, out_stride, s);
    ctx->scratch_busy = false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap == hipStreamCaptureStatusNone) { // (an event recorded inside a capture cannot be waited for outside it)
        WS_HIP(ctx, hipEventRecord(ctx->ev_scratch, s));
        ctx->scratch_busy = true;
        ctx->scratch_stream = s;
    }
    return rc;
}

// smoothFactor: for the right view and LinearSearch the factor can only reach d = 0 beside a
// zero-valued neighbour (see ws_smooth.hip), and only when d = 0 is a candidate at all.
int run_device_on(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R,
                  float *out, int out_stride, hipStream_t s)
{
    ws_params q = *p;
    if (q.view == WS_VIEW_LINEAR) q.min_disparity = 0;
    if (q.view == WS_VIEW_LEFT && q.smooth_factor != 1.0) {
        // the data-parallel search (smoothFactor 1) gives d1; the raster-order pass does the rest
        q.smooth_factor = 1.0;
        ctx->want_planes = true;
        int rc = run_search(ctx, &q, L, R, out, out_stride, s);
        ctx->want_planes = false;
        if (rc != WS_OK) return rc;
        GenericArgs ga = generic_args(p, L, R, out, out_stride);
        ga.min_d = 0;
        // per pixel the best candidate's cost (0 <= s <= 1) or the three best candidates
        if ((rc = ensure(ctx, ctx->top3, smooth_left_top_bytes(L->width, L->height, p->smooth_factor))) != WS_OK) return rc;
        uint32_t *top3 = static_cast<uint32_t *>(ctx->top3.p);
        WS_HIP(ctx, launch_smooth_left(ga, p->smooth_factor, top3, ctx->last_march && ctx->last_planes ? &ctx->last_canon : nullptr,
                                       ctx->last_pa, ctx->last_pb, ctx->status_dev, s));
        return WS_OK;
    }
    const bool smooth = q.smooth_factor != 1.0 && q.view != WS_VIEW_LEFT && q.min_disparity == 0;
    if (!smooth) return run_search(ctx, &q, L, R, out, out_stride, s);
    q.min_disparity = 1; // the data-parallel part: best candidate among d >= 1
    q.subpixel = 0;
    ctx->want_cost = p->view == WS_VIEW_RIGHT && !p->var_block;
    int rc = run_search(ctx, &q, L, R, out, out_stride, s);
    ctx->want_cost = false;
    if (rc != WS_OK) return rc;
    const int sel_pitch = (R->width + 63) & ~63;
    if ((rc = ensure(ctx, ctx->sel, (size_t)sel_pitch * (smooth_sel_rows(R->height) + 64))) != WS_OK) return rc;
    GenericArgs ga = generic_args(p, L, R, out, out_stride);
    ga.min_d = 0;
    if (p->view == WS_VIEW_RIGHT && p->var_block) { // the windows ws_varblock_kernel chose
        ga.bs_plane = static_cast<const int16_t *>(ctx->bs_plane.p);
        ga.bs_pitch = (R->width + 63) & ~63;
    }
    if ((rc = ensure(ctx, ctx->sel_planes, smooth_planes_bytes(R->width, R->height))) != WS_OK) return rc;
    const bool on_planes = p->view == WS_VIEW_RIGHT && !p->var_block && ctx->last_march && ctx->last_planes && ctx->last_cost;
    if (on_planes) {
        ga.skip_x0 = ctx->last_skip[0]; ga.skip_x1 = ctx->last_skip[1];
        ga.skip_y0 = ctx->last_skip[2]; ga.skip_y1 = ctx->last_skip[3];
    }
    WS_HIP(ctx, launch_smooth(ga, p->smooth_factor, static_cast<uint8_t *>(ctx->sel.p), sel_pitch,
                              static_cast<unsigned long long *>(ctx->sel_planes.p),
                              on_planes ? &ctx->last_canon : nullptr, ctx->last_pa, ctx->last_pb,
                              on_planes ? ctx->last_cost : nullptr, on_planes ? ctx->last_canon.wa : 0, s));
    if (p->subpixel) return fail(ctx, WS_ERR_UNSUPPORTED, "sub-pixel refinement together with smoothFactor != 1");
    return WS_OK;
}

int run_search(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R,
               float *out, int out_stride, hipStream_t s)
{
    const int ow = p->view == WS_VIEW_LEFT ? L->width : R->width;
    if (out_stride < ow) return fail(ctx, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);

    GenericArgs ga = generic_args(p, L, R, out, out_stride);
    ga.out16 = ctx->direct_i16;

    ctx->last_cost = nullptr;
    if (p->view == WS_VIEW_RIGHT) ctx->var_block_ran = false;
    if (p->view == WS_VIEW_RIGHT && p->var_block) {
        // the ordinary search first; then one wave per pixel decides the window (ws_varblock_kernel)
        // and searches again only where it grew
        ws_params q = *p;
        q.var_block = 0;
        q.subpixel = 0;
        int rc = run_search(ctx, &q, L, R, out, out_stride, s);
        if (rc != WS_OK) return rc;
        const int bs_pitch = (R->width + 63) & ~63;
        if ((rc = ensure(ctx, ctx->bs_plane, (size_t)bs_pitch * R->height * 2)) != WS_OK) return rc;
        if ((rc = ensure(ctx, ctx->max_block, 64)) != WS_OK) return rc;
        WS_HIP(ctx, launch_varblock(ga, p->thres, static_cast<int16_t *>(ctx->bs_plane.p), bs_pitch,
                                    static_cast<int *>(ctx->max_block.p), s));
        ctx->last_kernel = "ws_varblock_kernel";
        ctx->last_threads = 256;
        ctx->last_wgs = (int)(((long long)R->width * R->height + 3) / 4);
        ctx->last_lds = 0;
        ctx->var_block_ran = true;
        return WS_OK;
    }
    Canon c{};
    MarchLaunch m{};
    Plane ring_a{}, ring_b{};
    // (the plan of the last problem is kept: a queue of equal pairs asks for the same one every call, and the planner
    // walks every strip count for up to three candidate tilings and two workgroup sizes -- 5 us of a 15 us enqueue)
    bool march = make_canon(p, L, R, &c);
    if (march) {
        const int tune[3] = {ctx->tune_nxr, ctx->tune_rows, ctx->tune_threads};
        if (ctx->plan_valid && !memcmp(&ctx->plan_canon, &c, sizeof c) && !memcmp(ctx->plan_tune, tune, sizeof tune)) {
            m = ctx->plan_launch;
            march = ctx->plan_ok;
        } else {
            march = march_plan(c, ctx->num_cus, tune[0], tune[1], tune[2], &m);
            ctx->plan_canon = c;
            memcpy(ctx->plan_tune, tune, sizeof tune);
            ctx->plan_launch = m;
            ctx->plan_ok = march;
            ctx->plan_valid = true;
        }
    }
    // Dword planes of both images: only for the kernels BESIDE the marching kernel that still read them -- the right
    // view's border ring, the sub-pixel refine, the smoothFactor passes.  The marching kernel reads the caller's bytes.
    const bool planes = march && (p->view == WS_VIEW_RIGHT || p->subpixel || ctx->want_planes);
    if (march) {
        Plane pa{}, pb{};
        int rc;
        const ws_image *ia = p->view == WS_VIEW_LEFT ? L : R;
        const ws_image *ib = p->view == WS_VIEW_LEFT ? R : L;
        if (c.mirror) {
            ga.skip_x0 = c.wa - c.ox1; ga.skip_x1 = c.wa - c.ox0;
        } else {
            ga.skip_x0 = c.ox0; ga.skip_x1 = c.ox1;
        }
        ga.skip_y0 = c.oy0; ga.skip_y1 = c.oy1;
        if (planes) {
            march_plane_geometry(c, m, &pa, &pb);
            if ((rc = ensure(ctx, ctx->plane_a, (size_t)pa.pitch * c.ha * 4)) != WS_OK) return rc;
            if ((rc = ensure(ctx, ctx->plane_b, (size_t)pb.pitch * c.hb * 4)) != WS_OK) return rc;
            pa.data = static_cast<uint32_t *>(ctx->plane_a.p);
            pb.data = static_cast<uint32_t *>(ctx->plane_b.p);
            ring_a = pa;
            ring_b = pb;
            WS_HIP(ctx, launch_pack(c, ia->data, ia->stride, pa, ib->data, ib->stride, pb, s));
        }
        if (ctx->profiling) WS_HIP(ctx, hipEventRecord(ctx->evk0, s));
        const int keys_pitch = (c.wa + 15) & ~15;
        if (m.passes > 1 && (rc = ensure(ctx, ctx->keys, (size_t)keys_pitch * c.ha * 8)) != WS_OK) return rc;
        int32_t *cost_out = nullptr; // the smoothFactor passes of the right view want the winners' costs
        if (ctx->want_cost && march_has_cost(c)) {
            if ((rc = ensure(ctx, ctx->cost, (size_t)c.wa * c.ha * 4)) != WS_OK) return rc;
            cost_out = static_cast<int32_t *>(ctx->cost.p);
        }
        ctx->last_cost = cost_out;
        // left view: the marching kernel also writes the zeros outside its interior (BlockSearch.cpp:33,36,38); the
        // right view's ring runs on the packed planes after it
        WS_HIP(ctx, launch_march(c, m, ia->data, ia->stride, ib->data, ib->stride, out, ctx->direct_i16, out_stride,
                                 p->view == WS_VIEW_LEFT, L->width, L->height, ctx->keys.p, keys_pitch, cost_out, c.wa, s));
        if (ctx->profiling) {
            WS_HIP(ctx, hipEventRecord(ctx->evk1, s));
            ctx->kernel_timed = true;
        }
        ctx->last_kernel = march_kernel_name(c, m);
        ctx->last_threads = m.threads;
        ctx->last_wgs = m.tiles * m.strips;
        ctx->last_lds = (int)m.lds_bytes;
    } else {
        // (launch_linear hands ranges beyond kLinearMaxRange to the brute-force kernel: name the one that runs)
        ctx->last_kernel = p->view == WS_VIEW_LINEAR && p->linear_range <= kLinearMaxRange ? "ws_linear_kernel" : "ws_generic_kernel";
        ctx->last_threads = 256;
        ctx->last_wgs = ((ow + 255) / 256) * (p->view == WS_VIEW_LEFT ? L->height : R->height);
        ctx->last_lds = 0;
    }
    // everything the marching kernel does not own: border ring, rows past min(h1,h2), or all of it
    if (march && p->view == WS_VIEW_RIGHT)
        WS_HIP(ctx, launch_ring(c, ring_a, ring_b, ga, out, out_stride, ctx->last_cost, c.wa, s));
    else if (!march && p->view == WS_VIEW_LINEAR)
        WS_HIP(ctx, launch_linear(ga, s));
    else if (!march)
        WS_HIP(ctx, launch_generic(ga, s));
    ctx->last_march = march;
    ctx->last_planes = planes;
    if (march) {
        ctx->last_canon = c; ctx->last_pa = ring_a; ctx->last_pb = ring_b;
        ctx->last_skip[0] = ga.skip_x0; ctx->last_skip[1] = ga.skip_x1;
        ctx->last_skip[2] = ga.skip_y0; ctx->last_skip[3] = ga.skip_y1;
    }
    if (p->subpixel) {
        if (march) WS_HIP(ctx, launch_refine_planes(c, m, ring_a, ring_b, out, out_stride, s));
        WS_HIP(ctx, launch_refine(ga, s)); // the pixels outside the marching interior (all of them without it)
    }
    return WS_OK;
}

// A search whose kernels only ever WRITE the map (smoothFactor 1, no sub-pixel refine, no varBlock: the marching
// kernel's flush, the border ring, LinearSearch, the brute force) can store it in the wire format itself.
bool writes_only(const ws_params *p) { return p->smooth_factor == 1.0 && !p->subpixel && !(p->var_block && p->view == WS_VIEW_RIGHT); }

// The wire format of a host call's map (see "WIRE FORMAT" above): 16-bit integers when the search kernels can store
// them themselves and every value fits.  Whatever the disparity range, a stored value is a difference of two columns
// of one image row or a +-x fallback (BlockSearch.cpp:82: x - cx with 0 <= cx < x; :174: cx - x with x <= cx < w1, or
// -x; LinearSearch.cpp:53: col - j), so |value| < max(w1, w2): images up to 32767 pixels wide fit.  Else float32.
int wire_for(const ws_params *p, const ws_image *L, const ws_image *R)
{
    const bool fits = L->width <= 32767 && R->width <= 32767;
    return writes_only(p) && fits ? kWireI16 : kWireF32;
}

// one search whose map ends up in wire format: in out16 (kWireI16: stored by the search kernels, scratch32 stays unused)
// or in scratch32 (kWireF32)
int run_device_wire(ws_context *ctx, const ws_params *p, const ws_image *L, const ws_image *R, float *scratch32, int16_t *out16,
                    int wire, int ow, hipStream_t s)
{
    ctx->direct_i16 = wire == kWireI16 ? out16 : nullptr;
    const int rc = run_device(ctx, p, L, R, scratch32, ow, s);
    ctx->direct_i16 = nullptr;
    return rc;
}

void out_dims(const ws_params *p, const ws_image *L, const ws_image *R, int *w, int *h)
{
    *w = p->view == WS_VIEW_LEFT ? L->width : R->width;
    *h = p->view == WS_VIEW_LEFT ? L->height : R->height;
}

// What the kernels flagged since the last check (the streams that carried them are idle: the caller synchronised).
int check_device_status(ws_context *ctx)
{
    if (!ctx->status_host || !ctx->status_host[0]) return WS_OK;
    ctx->status_host[0] = 0;
    return fail(ctx, WS_ERR_HIP, "the left view's smoothFactor raster pass gave up waiting for the band above it "
                                 "(ws_smooth_left_bands_kernel): the map is not valid");
}

// The end of a synchronous host call: the streams idle (after an error too: nothing may still be copying when the spans are
// released), staged downloads handed over -- or dropped if the call or a stream failed -- and a stream's error reported.
int finish_host_call(ws_context *ctx, int rc, HostSpan *sp, int count, std::initializer_list<hipStream_t> streams, const char *what)
{
    hipError_t es = hipSuccess;
    for (hipStream_t s : streams) {
        const hipError_t e = hipStreamSynchronize(s);
        if (es == hipSuccess) es = e;
    }
    if (rc != WS_OK || es != hipSuccess)
        for (int i = 0; i < count; ++i) sp[i].down.clear();
    spans_finish(sp, count);
    if (rc == WS_OK && es != hipSuccess) return fail(ctx, WS_ERR_HIP, "%s: %s", what, hipGetErrorString(es));
    return rc;
}

} // namespace

extern "C" {

int ws_version(void) { return WS_VERSION; }

void ws_params_default(ws_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->view = WS_VIEW_LEFT;
    p->cost = WS_COST_SSD;
    p->block_size = 7;
    p->min_disparity = 0;
    p->max_disparity = 64;
    p->smooth_factor = 1.0;
    p->var_block = 0;
    p->thres = 19.0;
    p->subpixel = 0;
    p->linear_range = 200;
}

int ws_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ws_create(int device, ws_context **out)
{
    if (!out) return WS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, WS_ERR_HIP, "no HIP device available (%s): this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, WS_ERR_ARG, "device %d out of range [0,%d)", device, n);
    ws_context *ctx = new (std::nothrow) ws_context();
    if (!ctx) return WS_ERR_NOMEM;
    ctx->device = device;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess ||
        (e = hipEventCreate(&ctx->evk0)) != hipSuccess || (e = hipEventCreate(&ctx->evk1)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->ev_scratch, hipEventDisableTiming)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[0].ev_h2d, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[0].ev_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[1].ev_h2d, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[1].ev_done, hipEventDisableTiming)) != hipSuccess) {
        fail(nullptr, WS_ERR_HIP, "ws_create: %s", hipGetErrorString(e));
        delete ctx;
        return WS_ERR_HIP;
    }
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    march_set_num_cus(ctx->num_cus);
    if ((e = hipHostMalloc(reinterpret_cast<void **>(&ctx->status_page.p), 64, hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->status_dev), ctx->status_page.p, 0)) != hipSuccess) {
        fail(nullptr, WS_ERR_HIP, "ws_create: %s", hipGetErrorString(e));
        ws_destroy(ctx);
        return WS_ERR_HIP;
    }
    ctx->status_host = reinterpret_cast<unsigned int *>(ctx->status_page.p);
    memset(ctx->status_host, 0, 64);
    *out = ctx;
    return WS_OK;
}

void ws_destroy(ws_context *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t s : {ctx->stream, ctx->copy_stream, ctx->down_stream})
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (hipEvent_t e : {ctx->ev0, ctx->ev1, ctx->evk0, ctx->evk1, ctx->ev_scratch, ctx->jobs[0].ev_h2d, ctx->jobs[0].ev_done,
                         ctx->jobs[1].ev_h2d, ctx->jobs[1].ev_done})
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < ws_context::kMaxBands; ++i)
        for (hipEvent_t e : {ctx->ev_band_up[i], ctx->ev_band_done[i], ctx->ev_band_down[i]})
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_mesh)
        if (e) (void)hipEventDestroy(e);
    // every buffer goes with its owner, on this device, with nothing using it.  A batch never waited for: its maps are NOT
    // handed over -- only ws_wait delivers, and a caller who abandoned the batch may have freed the buffers they go to
    delete ctx;
}

const char *ws_last_error(const ws_context *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int ws_validate(const ws_params *p, const ws_image *left, const ws_image *right)
{
    // same checks as the search calls, without touching a device (message via ws_last_error(NULL))
    return check_params(nullptr, p, left, right);
}

int ws_plan(const ws_params *p, const ws_image *left, const ws_image *right, int num_cus, ws_plan_info *out)
{
    if (!out) return WS_ERR_ARG;
    memset(out, 0, sizeof *out);
    int rc = check_params(nullptr, p, left, right);
    if (rc != WS_OK) return rc;
    Canon c{};
    MarchLaunch m{};
    if (make_canon(p, left, right, &c) && march_plan(c, num_cus > 0 ? num_cus : 256, 0, 0, 0, &m)) {
        out->marching = 1;
        out->x_per_thread = m.x_per_thread; out->d_per_thread = m.nd_per_thread;
        out->x_runs = m.nxr; out->d_chunks = m.nch; out->threads = m.threads;
        out->tiles = m.tiles; out->strips = m.strips; out->strip_rows = m.strip_rows;
        out->lds_bytes = (int)m.lds_bytes;
        out->interior_x0 = c.mirror ? c.wa - c.ox1 : c.ox0;
        out->interior_x1 = c.mirror ? c.wa - c.ox0 : c.ox1;
        out->interior_y0 = c.oy0; out->interior_y1 = c.oy1;
        out->passes = m.passes;
        out->tile_cols = m.tile_cols;
    }
    return WS_OK;
}

int ws_search_device(ws_context *ctx, const ws_params *p, const ws_image *left_dev,
                     const ws_image *right_dev, float *out_dev, int out_stride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = check_params(ctx, p, left_dev, right_dev);
    if (rc != WS_OK) return rc;
    if (!out_dev) return fail(ctx, WS_ERR_ARG, "null output");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return run_device(ctx, p, left_dev, right_dev, out_dev, out_stride, s);
}

// One boundary call in row bands.  A pixel's result depends on the image rows its window covers and on nothing
// else when smoothFactor == 1 (no raster dependency, no varBlock growth): the map's rows [y0, y1) are the interior
// rows of a search on the sub-images [y0 - half, y1 + half).  So the call is cut into K bands and three queues run
// beside each other: band k+1's image rows go up (copy_stream) while band k is searched (the context's stream) and
// band k-1's map rows come down (down_stream) -- PCIe is full duplex and the copy engines are idle during a search.
// The bytes that cross are the same as in the plain path; only their timing changes.  Results are identical
// (tests/test_gpu_parity.py::test_host_call_in_bands_equals_the_plain_call).
static int search_host_banded(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                              void *out, int out_dtype, int ow, int oh, int nb)
{
    const int half = (p->block_size - 1) / 2;
    const size_t lb = (size_t)left->width * 3, rb = (size_t)right->width * 3;
    const int H = oh; // (equal heights: the caller checked)
    int rc;
    if (!ctx->down_stream) WS_HIP(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
    for (int i = 0; i < nb; ++i)
        for (hipEvent_t *e : {&ctx->ev_band_up[i], &ctx->ev_band_done[i], &ctx->ev_band_down[i]})
            if (!*e) WS_HIP(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    // the caller's three buffers for the duration of the call (HostSpan: caller-pinned or staged; both images cross as
    // whole spans: the caller checked linear_span)
    HostSpan sp[3];
    if ((rc = ensure(ctx, ctx->d_left, image_span(sp[0], left, &ctx->h_left))) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_right, image_span(sp[1], right, &ctx->h_right))) != WS_OK) return rc;
    const int wire = wire_for(p, left, right);
    if ((rc = ensure(ctx, ctx->d_out, (size_t)ow * (H + 2 * half * nb) * 4)) != WS_OK) return rc;
    if (wire == kWireI16 && (rc = ensure(ctx, ctx->d_out16, (size_t)ow * (H + 2 * half * nb) * 2)) != WS_OK) return rc;
    const int esz = out_dtype == WS_OUT_F32 ? 4 : 8;
    uint8_t *dl = static_cast<uint8_t *>(ctx->d_left.p), *dr = static_cast<uint8_t *>(ctx->d_right.p);
    float *scratch = static_cast<float *>(ctx->d_out.p);
    sp[2].p = static_cast<uint8_t *>(out); sp[2].n = (size_t)ow * H * esz; sp[2].stage = &ctx->h_out;
    HostTrace tr;
    spans_attach(sp, 3);
    tr.mark("attached");
    rc = [&]() -> int {
    int up_to = 0; // image rows [0, up_to) are on their way up
    for (int k = 0; k < nb; ++k) {
        // the first band's upload and the last band's download are what nothing can hide: those two bands are
        // half as tall as the others (nb >= 3)
        auto cut = [&](int i) -> int {
            if (nb < 3) return (int)((long long)H * i / nb);
            const long long units = 2LL * nb - 2; // 1 + 2 (nb - 2) + 1 half-bands
            const long long u = i == 0 ? 0 : i == nb ? units : 2LL * i - 1;
            return (int)(H * u / units);
        };
        const int y0 = cut(k), y1 = cut(k + 1);
        const int a = std::max(0, y0 - half), b = std::min(H, y1 + half);
        if (b > up_to) { // the rows this band adds: one linear copy per image, row padding included
            const size_t ol = (size_t)up_to * left->stride, orr = (size_t)up_to * right->stride;
            const size_t nl = (size_t)(b - 1 - up_to) * left->stride + lb, nr = (size_t)(b - 1 - up_to) * right->stride + rb;
            WS_HIP(ctx, span_upload(sp[0], ol, dl + ol, nl, ctx->copy_stream));
            WS_HIP(ctx, span_upload(sp[1], orr, dr + orr, nr, ctx->copy_stream));
            up_to = b;
        }
        tr.mark("up", k);
        WS_HIP(ctx, hipEventRecord(ctx->ev_band_up[k], ctx->copy_stream));
        WS_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_band_up[k], 0));
        ws_image bl{dl + (size_t)a * left->stride, left->width, b - a, left->stride};
        ws_image br{dr + (size_t)a * right->stride, right->width, b - a, right->stride};
        float *bout = scratch + (size_t)ow * (a + 2 * half * k); // the band's own map: its border rows are scrap
        int16_t *bout16 = wire == kWireI16 ? static_cast<int16_t *>(ctx->d_out16.p) + (size_t)ow * (a + 2 * half * k) : nullptr;
        if ((rc = run_device_wire(ctx, p, &bl, &br, bout, bout16, wire, ow, ctx->stream)) != WS_OK) return rc;
        const void *src = wire == kWireI16 ? static_cast<const void *>(bout16 + (size_t)ow * (y0 - a)) : static_cast<const void *>(bout + (size_t)ow * (y0 - a));
        WS_HIP(ctx, hipEventRecord(ctx->ev_band_done[k], ctx->stream));
        WS_HIP(ctx, hipStreamWaitEvent(ctx->down_stream, ctx->ev_band_done[k], 0));
        WS_HIP(ctx, span_download(sp[2], (size_t)ow * y0, (size_t)ow, src, (size_t)ow, (size_t)(y1 - y0), wire, esz, ctx->down_stream));
        WS_HIP(ctx, hipEventRecord(ctx->ev_band_down[k], ctx->down_stream));
        tr.mark("enq", k);
    }
    // a staged map: every band's rows go from the stage to the caller's buffer -- widened on the way -- as soon as they
    // are down, while the bands behind it are still being searched (segment k of the span is band k's download).
    // (Handing a band over earlier, between two later bands' uploads, measured 3 % slower: profiles/r04/host_trace.txt.)
    if (sp[2].down.size() == (size_t)nb) {
        for (int k = 0; k < nb; ++k) {
            WS_HIP(ctx, hipEventSynchronize(ctx->ev_band_down[k]));
            tr.mark("down", k);
            span_scatter_seg(sp[2], sp[2].down[(size_t)k]);
            tr.mark("out", k);
        }
    }
    return WS_OK;
    }();
    for (int i = 0; i < 3; ++i) ctx->last_how[i] = (int)sp[i].how;
    ctx->last_wire = wire;
    rc = finish_host_call(ctx, rc, sp, 3, {ctx->copy_stream, ctx->stream, ctx->down_stream}, "banded host call");
    return rc == WS_OK ? check_device_status(ctx) : rc;
}

int ws_device_status(ws_context *ctx, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    WS_HIP(ctx, hipSetDevice(ctx->device));
    WS_HIP(ctx, hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    return check_device_status(ctx);
}

int ws_last_host_paths(const ws_context *ctx, int how[3])
{
    if (!ctx || !how) return WS_ERR_ARG;
    for (int i = 0; i < 3; ++i) how[i] = ctx->last_how[i];
    return WS_OK;
}

int ws_last_wire_format(const ws_context *ctx, int *wire)
{
    if (!ctx || !wire) return WS_ERR_ARG;
    *wire = ctx->last_wire;
    return WS_OK;
}

int ws_last_outliers_path(const ws_context *ctx, int *path)
{
    if (!ctx || !path) return WS_ERR_ARG;
    *path = ctx->last_outliers_path;
    return WS_OK;
}

int ws_set_host_bands(ws_context *ctx, int bands)
{
    if (!ctx || bands < -1 || bands > ws_context::kMaxBands) return WS_ERR_ARG;
    ctx->host_bands = bands;
    return WS_OK;
}

int ws_search_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                   void *out, int out_stride, int out_dtype)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = check_params(ctx, p, left, right);
    if (rc != WS_OK) return rc;
    if (!out || (out_dtype != WS_OUT_F32 && out_dtype != WS_OUT_F64)) return fail(ctx, WS_ERR_ARG, "bad output");
    int ow, oh;
    out_dims(p, left, right, &ow, &oh);
    if (out_stride < ow) return fail(ctx, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    {
        // bands pay when the copies are worth hiding and each band still fills the chip
        const bool can = (p->view == WS_VIEW_LEFT || p->view == WS_VIEW_RIGHT) && p->smooth_factor == 1.0 && !p->var_block &&
                         left->height == right->height && out_stride == ow && linear_span(left) && linear_span(right) &&
                         (size_t)left->stride <= 2 * (size_t)left->width * 3 && (size_t)right->stride <= 2 * (size_t)right->width * 3;
        int nb = ctx->host_bands;
        // (measured on one MI355X, tools/host_bands_time.py: 1.5 Mpixel 0.61 -> 0.47 ms with 2..4 bands,
        // 5.9 Mpixel 2.6 -> 1.5 ms with 5..6; below a megapixel the bands' fixed costs eat the overlap)
        const size_t px = (size_t)ow * oh;
        if (nb < 0) nb = px < ((size_t)1 << 20) ? 0 : px < 3000000 ? 2 : px < 5000000 ? 4 : 6;
        if (can && nb >= 2 && oh >= 64 * nb) return search_host_banded(ctx, p, left, right, out, out_dtype, ow, oh, nb);
    }
    // The caller's buffers for the duration of the call (HostSpan): caller-pinned or staged -- every
    // host copy of this library goes the same way, whatever the band setting of the moment, and none through the
    // runtime's pageable path.
    HostSpan sp[3];
    if ((rc = ensure(ctx, ctx->d_left, image_span(sp[0], left, &ctx->h_left))) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_right, image_span(sp[1], right, &ctx->h_right))) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out, (size_t)ow * oh * 4)) != WS_OK) return rc;
    const int esz = out_dtype == WS_OUT_F32 ? 4 : 8;
    const int wire = wire_for(p, left, right);
    if (wire == kWireI16 && (rc = ensure(ctx, ctx->d_out16, (size_t)ow * oh * 2)) != WS_OK) return rc;
    sp[2].p = static_cast<uint8_t *>(out); sp[2].n = ((size_t)out_stride * (oh - 1) + ow) * esz; sp[2].stage = &ctx->h_out;
    spans_attach(sp, 3);
    rc = [&]() -> int {
        ws_image dl, dr;
        WS_HIP(ctx, upload_image(sp[0], left, static_cast<uint8_t *>(ctx->d_left.p), s, &dl));
        WS_HIP(ctx, upload_image(sp[1], right, static_cast<uint8_t *>(ctx->d_right.p), s, &dr));
        float *dout = static_cast<float *>(ctx->d_out.p);
        int16_t *dout16 = wire == kWireI16 ? static_cast<int16_t *>(ctx->d_out16.p) : nullptr;
        int rc2;
        if ((rc2 = run_device_wire(ctx, p, &dl, &dr, dout, dout16, wire, ow, s)) != WS_OK) return rc2;
        const void *src = wire == kWireI16 ? static_cast<const void *>(dout16) : static_cast<const void *>(dout);
        WS_HIP(ctx, span_download(sp[2], 0, (size_t)out_stride, src, (size_t)ow, (size_t)oh, wire, esz, s));
        return WS_OK;
    }();
    for (int i = 0; i < 3; ++i) ctx->last_how[i] = (int)sp[i].how;
    ctx->last_wire = wire;
    rc = finish_host_call(ctx, rc, sp, 3, {s}, "host call");
    return rc == WS_OK ? check_device_status(ctx) : rc;
}

// The batched host path keeps two pairs in flight: while one is searched (context stream) the next
// one's images go up and the previous one's map comes down on a second stream, straight from / to
// the caller's buffers as linear copies (see ws_search_host).
static int flush_job(ws_context *ctx, Job &j)
{
    if (!j.pending) return WS_OK;
    j.pending = false;
    WS_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, j.ev_done, 0));
    const int esz = j.dtype == WS_OUT_F32 ? 4 : 8;
    const size_t first = (size_t)j.row0 * j.w;
    const void *src = j.wire == kWireI16 ? static_cast<const void *>(static_cast<const int16_t *>(j.out16.p) + first)
                                         : static_cast<const void *>(static_cast<const float *>(j.out.p) + first);
    WS_HIP(ctx, span_download(ctx->batch_spans[(size_t)j.out_span], 0, (size_t)j.out_stride, src, (size_t)j.w, (size_t)j.h, j.wire, esz,
                              ctx->copy_stream));
    return WS_OK;
}

int ws_enqueue_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                    void *out, int out_stride, int out_dtype)
{
    return wsamd::enqueue_host_rows(ctx, p, left, right, out, out_stride, out_dtype, 0, -1);
}

} // extern "C"

// ws_enqueue_host of the rows [map_row0, map_row0 + map_rows) of the pair's map only (map_rows < 0: all of them):
// `out` is where map row map_row0 lands.  A row band of a bigger pair (ws_batch_search_host) is the search of its
// sub-images, halo rows included; only the band's own rows come down, so neighbouring bands never write each other's.
int wsamd::enqueue_host_rows(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, void *out,
                             int out_stride, int out_dtype, int map_row0, int map_rows)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = check_params(ctx, p, left, right);
    if (rc != WS_OK) return rc;
    if (!out || (out_dtype != WS_OUT_F32 && out_dtype != WS_OUT_F64)) return fail(ctx, WS_ERR_ARG, "bad output");
    int ow, oh;
    out_dims(p, left, right, &ow, &oh);
    if (out_stride < ow) return fail(ctx, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    if (map_rows < 0) {
        map_row0 = 0;
        map_rows = oh;
    }
    if (map_row0 < 0 || map_rows < 1 || map_row0 + map_rows > oh)
        return fail(ctx, WS_ERR_ARG, "map rows [%d, %d) outside [0, %d)", map_row0, map_row0 + map_rows, oh);
    WS_HIP(ctx, hipSetDevice(ctx->device));
    Job &job = ctx->jobs[ctx->job_next];
    Job &prev = ctx->jobs[ctx->job_next ^ 1];
    if ((rc = flush_job(ctx, job)) != WS_OK) return rc; // (only after an error left it pending)
    // this slot's previous pair: a map that came down through the slot's stage goes to its caller now, before the
    // stage is used again
    if (job.out_span >= 0 && !ctx->batch_spans[(size_t)job.out_span].down.empty()) {
        WS_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
        span_scatter(ctx->batch_spans[(size_t)job.out_span]);
    }
    job.out_span = -1;
    // The caller's buffers for the life of the batch (HostSpan; ws_wait hands the last maps over): pageable buffers cross
    // through the job slots' pinned stages (a host copy each way), buffers the caller pinned itself cross directly.
    HostSpan sp[3];
    const size_t span_l = image_span(sp[0], left, &job.h_left), span_r = image_span(sp[1], right, &job.h_right);
    const size_t off_r = (span_l + 255) & ~(size_t)255;
    const size_t out_elems = (size_t)ow * oh;
    // (hipFree waits for the device: nothing still reads a buffer that ensure replaces)
    if ((rc = ensure(ctx, job.in, off_r + span_r)) != WS_OK || (rc = ensure(ctx, job.out, out_elems * 4)) != WS_OK ||
        (rc = ensure(ctx, job.out16, out_elems * 2)) != WS_OK)
        return rc;
    uint8_t *d_left = static_cast<uint8_t *>(job.in.p), *d_right = d_left + off_r;
    hipStream_t cs = ctx->copy_stream;
    const int esz = out_dtype == WS_OUT_F32 ? 4 : 8;
    sp[2].p = static_cast<uint8_t *>(out); sp[2].n = ((size_t)out_stride * (map_rows - 1) + ow) * esz; sp[2].stage = &job.h_out;
    spans_attach(sp, 3);
    const size_t first = ctx->batch_spans.size();
    for (int i = 0; i < 3; ++i) ctx->batch_spans.push_back(sp[i]);
    HostSpan *bs = ctx->batch_spans.data() + first; // (valid until the next push_back: only used inside this call)
    job.out_span = (int)first + 2;
    // bytes that cross through this slot's pinned buffers (gathered cut-outs, stages): the slot's previous upload from
    // them must be through
    if (bs[0].how != HostSpan::kCallerPinned || bs[1].how != HostSpan::kCallerPinned) WS_HIP(ctx, hipEventSynchronize(job.ev_h2d));
    ws_image dl, dr;
    WS_HIP(ctx, upload_image(bs[0], left, d_left, cs, &dl));
    WS_HIP(ctx, upload_image(bs[1], right, d_right, cs, &dr));
    WS_HIP(ctx, hipEventRecord(job.ev_h2d, cs));
    WS_HIP(ctx, hipStreamWaitEvent(ctx->stream, job.ev_h2d, 0));
    job.wire = wire_for(p, left, right);
    if ((rc = run_device_wire(ctx, p, &dl, &dr, static_cast<float *>(job.out.p), static_cast<int16_t *>(job.out16.p), job.wire, ow,
                              ctx->stream)) != WS_OK)
        return rc;
    WS_HIP(ctx, hipEventRecord(job.ev_done, ctx->stream));
    job.user_out = out; job.w = ow; job.h = map_rows; job.row0 = map_row0; job.out_stride = out_stride; job.dtype = out_dtype;
    job.pending = true;
    ctx->job_next ^= 1;
    // the previous pair's map goes down while this one is searched
    return flush_job(ctx, prev);
}

extern "C" {

int ws_wait(ws_context *ctx)
{
    if (!ctx) return WS_ERR_ARG;
    WS_HIP(ctx, hipSetDevice(ctx->device));
    int rc = flush_job(ctx, ctx->jobs[ctx->job_next]); // the older one first
    if (rc == WS_OK) rc = flush_job(ctx, ctx->jobs[ctx->job_next ^ 1]);
    for (Job &j : ctx->jobs) j.pending = false; // (after an error nothing stays queued for a later batch)
    if (ctx->batch_spans.size() >= 3)
        for (int i = 0; i < 3; ++i) ctx->last_how[i] = (int)ctx->batch_spans[ctx->batch_spans.size() - 3 + (size_t)i].how;
    // (a pair whose flush failed never reached the stage: the maps that did are handed over unless a stream failed)
    const int rs = finish_host_call(ctx, WS_OK, ctx->batch_spans.data(), (int)ctx->batch_spans.size(), {ctx->copy_stream, ctx->stream}, "ws_wait");
    ctx->batch_spans.clear();
    ctx->jobs[0].out_span = ctx->jobs[1].out_span = -1;
    if (rs != WS_OK) return rs;
    return rc == WS_OK ? check_device_status(ctx) : rc;
}

static bool invert3x3(const double m[9], double out[9])
{
    // closed form (adjugate / determinant), as cv::invert does for 3x3 matrices
    const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                     m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (d == 0.0) return false;
    const double r = 1.0 / d;
    out[0] = (m[4] * m[8] - m[5] * m[7]) * r;
    out[1] = (m[2] * m[7] - m[1] * m[8]) * r;
    out[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    out[3] = (m[5] * m[6] - m[3] * m[8]) * r;
    out[4] = (m[0] * m[8] - m[2] * m[6]) * r;
    out[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    out[6] = (m[3] * m[7] - m[4] * m[6]) * r;
    out[7] = (m[1] * m[6] - m[0] * m[7]) * r;
    out[8] = (m[0] * m[4] - m[1] * m[3]) * r;
    return true;
}

int ws_warp_nearest_device(ws_context *ctx, const float *src_dev, int src_w, int src_h, int src_stride,
                           const double m[9], float *dst_dev, int dst_w, int dst_h, int dst_stride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    if (!src_dev || !dst_dev || !m || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 ||
        src_stride < src_w || dst_stride < dst_w)
        return fail(ctx, WS_ERR_ARG, "bad warp arguments");
    double inv[9];
    if (!invert3x3(m, inv)) return fail(ctx, WS_ERR_ARG, "singular warp matrix");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    WS_HIP(ctx, launch_warp(src_dev, src_w, src_h, src_stride, dst_dev, dst_w, dst_h, dst_stride, inv, s));
    return WS_OK;
}

int ws_warp_nearest_host(ws_context *ctx, const double *src, int src_w, int src_h, int src_stride,
                         const double m[9], double *dst, int dst_w, int dst_h, int dst_stride)
{
    if (!ctx) return WS_ERR_ARG;
    if (!src || !dst || !m || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 || src_stride < src_w ||
        dst_stride < dst_w)
        return fail(ctx, WS_ERR_ARG, "bad warp arguments");
    // disparity maps are integer valued (or f32 sub-pixel): f32 on the device, CV_64F at the boundary; the floats
    // cross from / to pinned memory of the library's own
    WS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)src_w * src_h, nd = (size_t)dst_w * dst_h;
    WS_HIP(ctx, host_ensure(ctx->h_left, ns * 4));
    WS_HIP(ctx, host_ensure(ctx->h_right, nd * 4));
    float *hs = reinterpret_cast<float *>(ctx->h_left.p), *hd = reinterpret_cast<float *>(ctx->h_right.p);
    for (int y = 0; y < src_h; ++y)
        for (int x = 0; x < src_w; ++x) hs[(size_t)y * src_w + x] = (float)src[(size_t)y * src_stride + x];
    int rc;
    if ((rc = ensure(ctx, ctx->d_out, ns * 4)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out64, nd * 4)) != WS_OK) return rc;
    WS_HIP(ctx, hipMemcpyAsync(ctx->d_out.p, hs, ns * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = ws_warp_nearest_device(ctx, static_cast<const float *>(ctx->d_out.p), src_w, src_h, src_w, m,
                                static_cast<float *>(ctx->d_out64.p), dst_w, dst_h, dst_w, ctx->stream);
    if (rc != WS_OK) return rc;
    WS_HIP(ctx, hipMemcpyAsync(hd, ctx->d_out64.p, nd * 4, hipMemcpyDeviceToHost, ctx->stream));
    WS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int y = 0; y < dst_h; ++y)
        for (int x = 0; x < dst_w; ++x) dst[(size_t)y * dst_stride + x] = (double)hd[(size_t)y * dst_w + x];
    return WS_OK;
}

// ---- rectification (src/Rectification/rectification.cpp) ------------------------------

// rectification.cpp:436-483: perspectiveTransform of the four corners (x' = (x*m0 + y*m1 + m2) * (1/w),
// w = x*m6 + y*m7 + m8), then the extent truncated to int.  perspectiveTransform puts a corner with |w| <= FLT_EPSILON
// at (0,0); such a homography sends the image to infinity and is refused instead.
int ws_rectified_size(const double H[9], int width, int height, int *out_w, int *out_h)
{
    if (!H || !out_w || !out_h || width <= 0 || height <= 0) return fail(nullptr, WS_ERR_ARG, "bad rectified-size arguments");
    const double cx[4] = {0.0, (double)width, (double)width, 0.0}, cy[4] = {0.0, 0.0, (double)height, (double)height};
    double min_x = INFINITY, min_y = INFINITY, max_x = -INFINITY, max_y = -INFINITY;
    for (int j = 0; j < 4; ++j) {
        double w = cx[j] * H[6] + cy[j] * H[7] + H[8];
        if (!(fabs(w) > FLT_EPSILON)) return fail(nullptr, WS_ERR_GEOMETRY, "corner %d maps to infinity (|w| <= FLT_EPSILON)", j);
        w = 1.0 / w;
        const double X = (cx[j] * H[0] + cy[j] * H[1] + H[2]) * w, Y = (cx[j] * H[3] + cy[j] * H[4] + H[5]) * w;
        min_x = std::min(X, min_x); max_x = std::max(X, max_x);
        min_y = std::min(Y, min_y); max_y = std::max(Y, max_y);
    }
    const double cols = max_x - min_x, rows = max_y - min_y;
    // (int) truncates: a size in [1, 32767] is an extent in [1, 32768)
    if (!(cols >= 1.0 && cols < 32768.0 && rows >= 1.0 && rows < 32768.0))
        return fail(nullptr, WS_ERR_GEOMETRY, "rectified size %g x %g outside [1, 32767]", cols, rows);
    *out_w = (int)cols;
    *out_h = (int)rows;
    return WS_OK;
}

int ws_rectify_device(ws_context *ctx, const ws_image *src_dev, const double H[9], uint8_t *dst_dev, int dst_w, int dst_h,
                      int dst_stride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    if (!image_ok(src_dev) || !H || !dst_dev || dst_w <= 0 || dst_h <= 0 || (long long)dst_stride < 3LL * dst_w)
        return fail(ctx, WS_ERR_ARG, "bad rectify arguments");
    double inv[9];
    if (!invert3x3(H, inv)) return fail(ctx, WS_ERR_ARG, "singular warp matrix");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    WS_HIP(ctx, launch_rectify(src_dev->data, src_dev->width, src_dev->height, src_dev->stride, inv, dst_dev, dst_w, dst_h,
                               dst_stride, s));
    return WS_OK;
}

// ImageRectifier: rectifyImagesAndKeyPoints (images) + computeDisparityMapLeft/Right, on the context stream: the
// originals go up as in ws_search_host, both are rectified into context scratch, searched by the same device path, the
// rectified map is warped back with H_.inv() (nearest) and comes down as float32, widened to the caller's type on the
// host.  One synchronisation at the end.
int ws_search_unrectified_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                               const double H[9], const double Hp[9], void *out, int out_stride, int out_dtype,
                               uint8_t *rect_left, int rect_left_stride, uint8_t *rect_right, int rect_right_stride)
{
    if (!ctx) return WS_ERR_ARG;
    if (!p || !image_ok(left) || !image_ok(right) || !H || !Hp) return fail(ctx, WS_ERR_ARG, "null or malformed image / params / homography");
    if (p->view == WS_VIEW_LINEAR) return fail(ctx, WS_ERR_ARG, "ImageRectifier has no LinearSearch method");
    if (!out || (out_dtype != WS_OUT_F32 && out_dtype != WS_OUT_F64)) return fail(ctx, WS_ERR_ARG, "bad output");
    double h_inv[9], hp_inv[9], back[9]; // M^-1 of the two forward warps; M^-1 of the warp back, M = H_.inv()
    if (!invert3x3(H, h_inv) || !invert3x3(Hp, hp_inv) || !invert3x3(h_inv, back)) return fail(ctx, WS_ERR_ARG, "singular homography");
    int lw, lh, rw, rh, rc;
    if ((rc = ws_rectified_size(H, left->width, left->height, &lw, &lh)) != WS_OK ||
        (rc = ws_rectified_size(Hp, right->width, right->height, &rw, &rh)) != WS_OK)
        return fail(ctx, rc, "%s", ws_last_error(nullptr));
    const ws_image shape_l{left->data, lw, lh, 3 * lw}, shape_r{right->data, rw, rh, 3 * rw};
    if ((rc = check_params(ctx, p, &shape_l, &shape_r)) != WS_OK) return rc;
    const bool lv = p->view == WS_VIEW_LEFT;
    const int ow = lv ? left->width : right->width, oh = lv ? left->height : right->height; // the original frame
    const int mw = lv ? lw : rw, mh = lv ? lh : rh;                                         // the rectified map
    if (out_stride < ow) return fail(ctx, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    if ((rect_left && rect_left_stride < 3 * lw) || (rect_right && rect_right_stride < 3 * rw))
        return fail(ctx, WS_ERR_ARG, "rectified image stride below 3 * width");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the caller's buffers for the duration of the call (HostSpan, like ws_search_host)
    HostSpan sp[5];
    if ((rc = ensure(ctx, ctx->d_left, image_span(sp[0], left, &ctx->h_left))) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_right, image_span(sp[1], right, &ctx->h_right))) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_rect_left, (size_t)lw * lh * 3)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_rect_right, (size_t)rw * rh * 3)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out, (size_t)mw * mh * 4)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out64, (size_t)ow * oh * 4)) != WS_OK) return rc;
    const int esz = out_dtype == WS_OUT_F32 ? 4 : 8;
    sp[2].p = static_cast<uint8_t *>(out); sp[2].n = ((size_t)out_stride * (oh - 1) + ow) * esz; sp[2].stage = &ctx->h_out;
    if (rect_left) { sp[3].p = rect_left; sp[3].n = (size_t)rect_left_stride * (lh - 1) + 3 * (size_t)lw; sp[3].stage = &ctx->h_aux[0]; }
    if (rect_right) { sp[4].p = rect_right; sp[4].n = (size_t)rect_right_stride * (rh - 1) + 3 * (size_t)rw; sp[4].stage = &ctx->h_aux[1]; }
    spans_attach(sp, 5);
    uint8_t *drl = static_cast<uint8_t *>(ctx->d_rect_left.p), *drr = static_cast<uint8_t *>(ctx->d_rect_right.p);
    rc = [&]() -> int {
        ws_image dl, dr;
        WS_HIP(ctx, upload_image(sp[0], left, static_cast<uint8_t *>(ctx->d_left.p), s, &dl));
        WS_HIP(ctx, upload_image(sp[1], right, static_cast<uint8_t *>(ctx->d_right.p), s, &dr));
        // warpPerspective(leftImage_, .., H_, size), warpPerspective(rightImage_, .., Hp_, size) (rectification.cpp:486-493)
        WS_HIP(ctx, launch_rectify(dl.data, dl.width, dl.height, dl.stride, h_inv, drl, lw, lh, 3 * lw, s));
        WS_HIP(ctx, launch_rectify(dr.data, dr.width, dr.height, dr.stride, hp_inv, drr, rw, rh, 3 * rw, s));
        // BlockSearch on the rectified pair (rectification.cpp:67-68, :79-80)
        const ws_image il{drl, lw, lh, 3 * lw}, ir{drr, rw, rh, 3 * rw};
        float *rect_map = static_cast<float *>(ctx->d_out.p), *map = static_cast<float *>(ctx->d_out64.p);
        int rc2;
        if ((rc2 = run_device_wire(ctx, p, &il, &ir, rect_map, nullptr, kWireF32, mw, s)) != WS_OK) return rc2;
        // cv::warpPerspective(disparityMap_rect, .., H_.inv(), original size, INTER_NEAREST) (rectification.cpp:70-75, :82-87)
        WS_HIP(ctx, launch_warp(rect_map, mw, mh, mw, map, ow, oh, ow, back, s));
        WS_HIP(ctx, span_download(sp[2], 0, (size_t)out_stride, map, (size_t)ow, (size_t)oh, kWireF32, esz, s));
        if (rect_left) WS_HIP(ctx, span_download_bytes(sp[3], 0, (size_t)rect_left_stride, drl, 3 * (size_t)lw, (size_t)lh, s));
        if (rect_right) WS_HIP(ctx, span_download_bytes(sp[4], 0, (size_t)rect_right_stride, drr, 3 * (size_t)rw, (size_t)rh, s));
        return WS_OK;
    }();
    rc = finish_host_call(ctx, rc, sp, 5, {s}, "unrectified host call");
    return rc == WS_OK ? check_device_status(ctx) : rc;
}

// ---- consumers of the map (src/Reconstruction/reconstruction.cpp) ----------------------

int ws_remove_disparity_outliers(ws_context *ctx, float *map, int width, int height, int stride, int kernel_size,
                                 float thr_front, float thr_back)
{
    if (!ctx) return WS_ERR_ARG;
    if (!map || width <= 0 || height <= 0 || stride < width || kernel_size < 1)
        return fail(ctx, WS_ERR_ARG, "bad removeDisparityOutliers arguments");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    int rc;
    if ((rc = ensure(ctx, ctx->d_out, n * 4)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out64, std::max(n * 8, outliers_u32_scratch_bytes(width, height, ctx->num_cus)))) != WS_OK) return rc;
    if (!ctx->d_flag.p) {
        if ((rc = ensure(ctx, ctx->d_flag, 256)) != WS_OK) return rc;
        WS_HIP(ctx, hipMemsetAsync(ctx->d_flag.p, 0, 256, s));
    }
    float *dmap = static_cast<float *>(ctx->d_out.p);
    // the caller's map for the duration of the call (HostSpan, like ws_search_host: no pageable copies)
    HostSpan sp[1];
    sp[0].p = reinterpret_cast<uint8_t *>(map); sp[0].n = ((size_t)stride * (height - 1) + width) * 4; sp[0].stage = &ctx->h_out;
    spans_attach(sp, 1);
    // 8-bit maps (the pipeline's PNG: integers in [0, 255]) take the 32-bit integer kernels; a map with any other value
    // raises status word 1, is left as uploaded, and goes through the double kernels after the first synchronisation
    const bool try_u32 = ctx->d_flag.p && outliers_u32_applies(width, height, kernel_size, ctx->num_cus);
    auto pass = [&](bool u32) -> int { // the kernels on the uploaded map, the result down to the caller's
        if (u32)
            WS_HIP(ctx, launch_outliers_u32(dmap, width, width, height, kernel_size, thr_front, thr_back, static_cast<uint32_t *>(ctx->d_out64.p),
                                            static_cast<uint32_t *>(ctx->d_flag.p), ctx->status_dev + 1, ctx->num_cus, s));
        else
            WS_HIP(ctx, launch_outliers(dmap, width, width, height, kernel_size, thr_front, thr_back, static_cast<double *>(ctx->d_out64.p), s));
        WS_HIP(ctx, span_download_bytes(sp[0], 0, (size_t)stride * 4, dmap, (size_t)width * 4, (size_t)height, s));
        return WS_OK;
    };
    rc = [&]() -> int {
        WS_HIP(ctx, span_upload_rows(sp[0], 0, (size_t)stride * 4, dmap, (size_t)width * 4, (size_t)height, s));
        return pass(try_u32);
    }();
    const hipError_t es = hipStreamSynchronize(s);
    ctx->last_outliers_path = try_u32 ? 1 : 0;
    if (rc == WS_OK && es != hipSuccess) rc = fail(ctx, WS_ERR_HIP, "removeDisparityOutliers: %s", hipGetErrorString(es));
    if (rc != WS_OK || !try_u32 || !ctx->status_host[1]) return finish_host_call(ctx, rc, sp, 1, {}, "removeDisparityOutliers");
    ctx->status_host[1] = 0;
    ctx->last_outliers_path = 2;
    rc = [&]() -> int {
        WS_HIP(ctx, hipMemsetAsync(ctx->d_flag.p, 0, 256, s));
        return pass(false);
    }();
    return finish_host_call(ctx, rc, sp, 1, {s}, "removeDisparityOutliers");
}

static int depth_vertices_host(ws_context *ctx, const float *in, int width, int height, int stride, int input_is_depth,
                               float focal, float baseline, const float *k, const ws_image *bgr, float *depth,
                               int depth_stride, float *positions, uint8_t *colors)
{
    if (!ctx) return WS_ERR_ARG;
    if (!in || width <= 0 || height <= 0 || stride < width) return fail(ctx, WS_ERR_ARG, "bad map");
    if (positions && (!colors || !k || !bgr || !bgr->data || bgr->width != width || bgr->height != height ||
                      bgr->stride < 3 * width))
        return fail(ctx, WS_ERR_ARG, "back-projection needs K, a colour image of the map's size and both outputs");
    WS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    int rc;
    if ((rc = ensure(ctx, ctx->d_out, n * 4)) != WS_OK) return rc;
    if ((rc = ensure(ctx, ctx->d_out64, n * 4 + n * 16 + n * 4)) != WS_OK) return rc;
    // the caller's buffers for the duration of the call (HostSpan, like ws_search_host: no pageable copies)
    HostSpan sp[5];
    if (positions && (rc = ensure(ctx, ctx->d_left, image_span(sp[4], bgr, &ctx->h_left))) != WS_OK) return rc;
    float *din = static_cast<float *>(ctx->d_out.p);
    uint8_t *base = static_cast<uint8_t *>(ctx->d_out64.p);
    float *dpos = reinterpret_cast<float *>(base);           // n * 16 bytes, 16-byte aligned
    float *ddepth = reinterpret_cast<float *>(base + n * 16); // n * 4
    uint8_t *dcol = base + n * 20;                            // n * 4
    sp[0].p = reinterpret_cast<uint8_t *>(const_cast<float *>(in)); sp[0].n = ((size_t)stride * (height - 1) + width) * 4; sp[0].stage = &ctx->h_out;
    if (depth) { sp[1].p = reinterpret_cast<uint8_t *>(depth); sp[1].n = ((size_t)depth_stride * (height - 1) + width) * 4; sp[1].stage = &ctx->h_right; }
    if (positions) {
        sp[2].p = reinterpret_cast<uint8_t *>(positions); sp[2].n = n * 16; sp[2].stage = &ctx->h_aux[0];
        sp[3].p = colors; sp[3].n = n * 4; sp[3].stage = &ctx->h_aux[1];
    }
    spans_attach(sp, 5);
    rc = [&]() -> int {
        WS_HIP(ctx, span_upload_rows(sp[0], 0, (size_t)stride * 4, din, (size_t)width * 4, (size_t)height, s));
        ws_image dbgr{static_cast<const uint8_t *>(ctx->d_left.p), width, height, width * 3};
        if (positions) WS_HIP(ctx, upload_image(sp[4], bgr, static_cast<uint8_t *>(ctx->d_left.p), s, &dbgr));
        WS_HIP(ctx, launch_depth_vertices(din, width, width, height, focal, baseline, k, dbgr.data, dbgr.stride, depth ? ddepth : nullptr, width,
                                          positions ? dpos : nullptr, positions ? dcol : nullptr, input_is_depth, s));
        if (depth) WS_HIP(ctx, span_download_bytes(sp[1], 0, (size_t)depth_stride * 4, ddepth, (size_t)width * 4, (size_t)height, s));
        if (positions) {
            WS_HIP(ctx, span_download_bytes(sp[2], 0, n * 16, dpos, n * 16, 1, s));
            WS_HIP(ctx, span_download_bytes(sp[3], 0, n * 4, dcol, n * 4, 1, s));
        }
        return WS_OK;
    }();
    return finish_host_call(ctx, rc, sp, 5, {s}, "depth / vertices");
}

int ws_convert_disparity_to_depth(ws_context *ctx, const float *disp, int width, int height, int stride, float focal_length,
                                  float baseline, float *depth, int depth_stride)
{
    if (!depth || depth_stride < width) return ctx ? fail(ctx, WS_ERR_ARG, "bad depth output") : WS_ERR_ARG;
    return depth_vertices_host(ctx, disp, width, height, stride, 0, focal_length, baseline, nullptr, nullptr, depth,
                               depth_stride, nullptr, nullptr);
}

int ws_back_project(ws_context *ctx, const float *depth, int width, int height, int stride, const float intrinsics[9],
                    const ws_image *bgr, float *positions, uint8_t *colors)
{
    if (!positions || !colors) return ctx ? fail(ctx, WS_ERR_ARG, "null vertex output") : WS_ERR_ARG;
    return depth_vertices_host(ctx, depth, width, height, stride, 1, 0.0f, 0.0f, intrinsics, bgr, nullptr, 0, positions, colors);
}

// ---- WriteMesh (reconstruction.cpp:72-149) on the device: the kernels of ws_mesh.hip lay out the file's text, the host
// only moves the finished bytes into the file ------------------------------------------------------------------------

static constexpr size_t kMeshChunk = 8u << 20; // the text comes down in chunks of this size: pinned memory stays 2 chunks

static int mesh_args(ws_context *ctx, const void *pos, const void *col, int width, int height, const char *path)
{
    if (!path) return fail(ctx, WS_ERR_ARG, "null mesh path");
    if (!pos || !col) return fail(ctx, WS_ERR_ARG, "null input buffer");
    if (width <= 0 || height <= 0) return fail(ctx, WS_ERR_ARG, "bad mesh size %d x %d", width, height);
    if ((uint64_t)width * (uint64_t)height > UINT32_MAX)
        return fail(ctx, WS_ERR_ARG, "a %d x %d mesh has more vertices than 32-bit indices reach", width, height);
    return WS_OK;
}

static FILE *mesh_open(ws_context *ctx, const char *path, int *rc)
{
    FILE *f = fopen(path, "wb");
    *rc = f ? WS_OK : fail(ctx, WS_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    return f;
}

// The end of a mesh call: the stream idle (a failed call may have copies in flight into the chunks), the file closed.
static int mesh_close(ws_context *ctx, int rc, FILE *f, hipStream_t s)
{
    if (rc != WS_OK) (void)hipStreamSynchronize(s);
    if (fclose(f) != 0 && rc == WS_OK) rc = fail(ctx, WS_ERR_IO, "closing the mesh file failed: %s", strerror(errno));
    return rc;
}

// The COFF text of the w x h vertices at dpos / dcol (device) -> the open file f; everything on stream s.  The kernels
// measure and lay out the text, one synchronisation fetches its size, the text comes down chunk by chunk through two
// pinned stages and each chunk is written while the next one is in flight.
static int mesh_to_file(ws_context *ctx, const float *dpos, const uint8_t *dcol, int w, int h, float thr, FILE *f, hipStream_t s)
{
    HostTrace tr; // WS_HOST_TRACE=1: when the text's size was known, time waited for chunks (the write kernel included), time writing
    const size_t nb = mesh_blocks(w, h);
    int rc;
    if ((rc = ensure(ctx, ctx->d_mesh, 64 + nb * 16)) != WS_OK) return rc;
    for (HostBuf &b : ctx->h_mesh) WS_HIP(ctx, host_ensure(b, kMeshChunk));
    for (hipEvent_t &e : ctx->ev_mesh)
        if (!e) WS_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint8_t *base = static_cast<uint8_t *>(ctx->d_mesh.p);
    auto *meta = reinterpret_cast<unsigned long long *>(base);             // {header bytes, file bytes, faces}
    auto *sums = reinterpret_cast<uint32_t *>(base + 64);                  // 2 words per workgroup
    auto *offs = reinterpret_cast<unsigned long long *>(base + 64 + nb * 8); // 1 word per workgroup
    WS_HIP(ctx, launch_mesh_count(dpos, dcol, w, h, thr, sums, offs, meta, s));
    WS_HIP(ctx, hipMemcpyAsync(ctx->h_mesh[0].p, meta, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    WS_HIP(ctx, hipStreamSynchronize(s));
    unsigned long long hm[3];
    memcpy(hm, ctx->h_mesh[0].p, sizeof hm);
    tr.mark("sized");
    const size_t bytes = (size_t)hm[1];
    if ((rc = ensure(ctx, ctx->d_mesh_text, bytes)) != WS_OK) return rc;
    const char *text = static_cast<const char *>(ctx->d_mesh_text.p);
    WS_HIP(ctx, launch_mesh_write(dpos, dcol, w, h, thr, offs, meta, static_cast<char *>(ctx->d_mesh_text.p), s));
    double us_wait = 0, us_write = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    int pending = -1; // the chunk that has been enqueued but not yet written to the file
    size_t pending_len = 0;
    for (size_t off = 0, k = 0; off < bytes || pending >= 0; ++k) {
        int cur = -1;
        size_t len = 0;
        if (off < bytes) {
            cur = (int)(k & 1);
            len = std::min(kMeshChunk, bytes - off);
            WS_HIP(ctx, hipMemcpyAsync(ctx->h_mesh[cur].p, text + off, len, hipMemcpyDeviceToHost, s));
            WS_HIP(ctx, hipEventRecord(ctx->ev_mesh[cur], s));
            off += len;
        }
        if (pending >= 0) {
            const auto t0 = now();
            WS_HIP(ctx, hipEventSynchronize(ctx->ev_mesh[pending]));
            const auto t1 = now();
            if (fwrite(ctx->h_mesh[pending].p, 1, pending_len, f) != pending_len)
                return fail(ctx, WS_ERR_IO, "writing the mesh file failed: %s", strerror(errno));
            us_wait += std::chrono::duration<double, std::micro>(t1 - t0).count();
            us_write += std::chrono::duration<double, std::micro>(now() - t1).count();
        }
        pending = cur;
        pending_len = len;
    }
    if (tr.on) {
        char buf[96];
        snprintf(buf, sizeof buf, " chunk_wait_total=%.0f fwrite_total=%.0f bytes=%zu", us_wait, us_write, bytes);
        tr.line += buf;
    }
    return WS_OK;
}

int ws_write_mesh_off_device(ws_context *ctx, const float *positions_dev, const uint8_t *colors_dev, int width, int height,
                             float edge_threshold, const char *path, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = mesh_args(ctx, positions_dev, colors_dev, width, height, path);
    if (rc != WS_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(positions_dev) & 15) || (reinterpret_cast<uintptr_t>(colors_dev) & 3))
        return fail(ctx, WS_ERR_ARG, "positions must be 16-byte aligned, colors 4-byte aligned");
    FILE *f = mesh_open(ctx, path, &rc);
    if (!f) return rc;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    rc = [&]() -> int {
        WS_HIP(ctx, hipSetDevice(ctx->device));
        return mesh_to_file(ctx, positions_dev, colors_dev, width, height, edge_threshold, f, s);
    }();
    return mesh_close(ctx, rc, f, s);
}

int ws_reconstruction_host(ws_context *ctx, const float *depth, int width, int height, int stride, const float intrinsics[9],
                           const ws_image *bgr, float edge_threshold, const char *path)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = mesh_args(ctx, depth, bgr, width, height, path);
    if (rc != WS_OK) return rc;
    if (stride < width) return fail(ctx, WS_ERR_ARG, "bad depth stride");
    if (!intrinsics || !bgr->data || bgr->width != width || bgr->height != height || bgr->stride < 3 * width)
        return fail(ctx, WS_ERR_ARG, "reconstruction needs K and a colour image of the depth map's size");
    FILE *f = mesh_open(ctx, path, &rc);
    if (!f) return rc;
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    // as ws_back_project, without the vertices' way down: depth and image go up (HostSpan), the vertices stay on the device
    HostSpan sp[2];
    rc = [&]() -> int {
        WS_HIP(ctx, hipSetDevice(ctx->device));
        int r;
        if ((r = ensure(ctx, ctx->d_out, n * 4)) != WS_OK) return r;
        if ((r = ensure(ctx, ctx->d_out64, n * 20)) != WS_OK) return r;
        return ensure(ctx, ctx->d_left, image_span(sp[1], bgr, &ctx->h_left));
    }();
    if (rc != WS_OK) return mesh_close(ctx, rc, f, s);
    float *din = static_cast<float *>(ctx->d_out.p);
    uint8_t *vbase = static_cast<uint8_t *>(ctx->d_out64.p);
    float *dpos = reinterpret_cast<float *>(vbase); // n * 16 bytes, 16-byte aligned
    uint8_t *dcol = vbase + n * 16;                 // n * 4
    sp[0].p = reinterpret_cast<uint8_t *>(const_cast<float *>(depth)); sp[0].n = ((size_t)stride * (height - 1) + width) * 4; sp[0].stage = &ctx->h_out;
    spans_attach(sp, 2);
    rc = [&]() -> int {
        WS_HIP(ctx, span_upload_rows(sp[0], 0, (size_t)stride * 4, din, (size_t)width * 4, (size_t)height, s));
        ws_image dbgr{static_cast<const uint8_t *>(ctx->d_left.p), width, height, width * 3};
        WS_HIP(ctx, upload_image(sp[1], bgr, static_cast<uint8_t *>(ctx->d_left.p), s, &dbgr));
        WS_HIP(ctx, launch_depth_vertices(din, width, width, height, 0.0f, 0.0f, intrinsics, dbgr.data, dbgr.stride, nullptr, width,
                                          dpos, dcol, 1, s));
        return mesh_to_file(ctx, dpos, dcol, width, height, edge_threshold, f, s);
    }();
    rc = finish_host_call(ctx, rc, sp, 2, {s}, "reconstruction");
    return mesh_close(ctx, rc, f, s);
}

int ws_timer_begin(ws_context *ctx, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    WS_HIP(ctx, hipSetDevice(ctx->device));
    WS_HIP(ctx, hipEventRecord(ctx->ev0, stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    return WS_OK;
}

int ws_timer_end(ws_context *ctx, void *stream, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return WS_ERR_ARG;
    WS_HIP(ctx, hipEventRecord(ctx->ev1, stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    WS_HIP(ctx, hipEventSynchronize(ctx->ev1));
    WS_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return WS_OK;
}

int ws_set_profiling(ws_context *ctx, int enable)
{
    if (!ctx) return WS_ERR_ARG;
    ctx->profiling = enable != 0;
    ctx->kernel_timed = false;
    return WS_OK;
}

int ws_last_kernel_ms(ws_context *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return WS_ERR_ARG;
    if (!ctx->kernel_timed) return fail(ctx, WS_ERR_ARG, "no marching-kernel launch was timed (ws_set_profiling off, or the generic path ran)");
    WS_HIP(ctx, hipEventSynchronize(ctx->evk1));
    WS_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->evk0, ctx->evk1));
    return WS_OK;
}

int ws_last_max_block(ws_context *ctx, int block_size, int *max_block)
{
    if (!ctx || !max_block) return WS_ERR_ARG;
    *max_block = block_size;
    if (!ctx->var_block_ran) return WS_OK;
    int v = 0;
    WS_HIP(ctx, hipSetDevice(ctx->device));
    WS_HIP(ctx, hipDeviceSynchronize());
    WS_HIP(ctx, hipMemcpy(&v, ctx->max_block.p, sizeof v, hipMemcpyDeviceToHost));
    if (v > block_size) *max_block = v;
    return WS_OK;
}

int ws_last_launch_info(const ws_context *ctx, char *kernel_name, int name_cap, int *threads,
                        int *workgroups, int *lds_bytes)
{
    if (!ctx) return WS_ERR_ARG;
    if (kernel_name && name_cap > 0) {
        strncpy(kernel_name, ctx->last_kernel.c_str(), (size_t)name_cap - 1);
        kernel_name[name_cap - 1] = 0;
    }
    if (threads) *threads = ctx->last_threads;
    if (workgroups) *workgroups = ctx->last_wgs;
    if (lds_bytes) *lds_bytes = ctx->last_lds;
    return WS_OK;
}

int ws_set_tuning(ws_context *ctx, int x_runs_per_tile, int strip_rows, int threads)
{
    if (!ctx || x_runs_per_tile < 0 || strip_rows < 0 || threads < 0) return WS_ERR_ARG;
    ctx->tune_nxr = x_runs_per_tile;
    ctx->tune_rows = strip_rows;
    ctx->tune_threads = threads;
    return WS_OK;
}

} // extern "C"
