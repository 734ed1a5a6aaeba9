// ws_capi.cpp -- the C-ABI of include/ws_stereo.h: the context, the entry points that run the search dispatch
// (ws_search.h) on device memory or on the caller's host buffers (through ws_staging.h), and the rectify, consumer and
// mesh calls.  Compiled with hipcc; no compute happens on the host.  The context is defined in ws_context.h; the
// left-right check's entry points are in ws_lr.cpp, the speckle filter's in ws_speckle.cpp.
// The Middlebury plumbing (PFM, calib.txt, evaldisp) is in ws_io.cpp.
#include "../../include/ws_stereo.h"
#include "ws_ct.h"
#include "ws_kernels.h"
#include "ws_rectify.h"
#include "ws_search.h"
#include "ws_staging.h"
#include "ws_context.h"

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

int wsamd::fail(std::string *err, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (err ? *err : g_create_error) = buf;
    return code;
}

int wsamd::check_device_status(ws_context *ctx)
{
    if (!ctx->status_host || !ctx->status_host[0]) return WS_OK;
    ctx->status_host[0] = 0;
    return fail(&ctx->err, WS_ERR_HIP, "the left view's smoothFactor raster pass gave up waiting for the band above it "
                                       "(ws_smooth_left_bands_kernel): the map is not valid");
}

int wsamd::finish_host_call(ws_context *ctx, int rc, HostSpan *sp, int count, std::initializer_list<hipStream_t> streams, const char *what)
{
    hipError_t es = hipSuccess;
    for (hipStream_t s : streams) {
        const hipError_t e = hipStreamSynchronize(s);
        if (es == hipSuccess) es = e;
    }
    if (rc != WS_OK || es != hipSuccess)
        for (int i = 0; i < count; ++i) sp[i].down.clear();
    spans_finish(sp, count);
    if (rc == WS_OK && es != hipSuccess) return fail(&ctx->err, WS_ERR_HIP, "%s: %s", what, hipGetErrorString(es));
    return rc;
}

int wsamd::PairHostCall::open()
{
    if (const int rc = ensure(&ctx->err, ctx->d_left, image_span(sp[0], left, &ctx->h_left)); rc != WS_OK) return rc;
    return ensure(&ctx->err, ctx->d_right, image_span(sp[1], right, &ctx->h_right));
}

int wsamd::PairHostCall::upload()
{
    WS_HIP(&ctx->err, upload_image(sp[0], left, static_cast<uint8_t *>(ctx->d_left.p), s, &dl));
    WS_HIP(&ctx->err, upload_image(sp[1], right, static_cast<uint8_t *>(ctx->d_right.p), s, &dr));
    return WS_OK;
}

int wsamd::PairHostCall::close(int rc, int count, int wire, bool device_status, const char *what, std::initializer_list<hipStream_t> streams)
{
    if (wire >= 0) {
        for (int i = 0; i < 3; ++i) ctx->last_how[i] = (int)sp[i].how;
        ctx->last_wire = wire;
    }
    rc = streams.size() ? finish_host_call(ctx, rc, sp, count, streams, what) : finish_host_call(ctx, rc, sp, count, {s}, what);
    return rc == WS_OK && device_status ? check_device_status(ctx) : rc;
}

int wsamd::read_counts(ws_context *ctx, CountPair &c, ScratchLease &lease, const char *none, unsigned long long out[2])
{
    if (!c.ran) return fail(&ctx->err, WS_ERR_ARG, "%s", none);
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    if (lease.busy) WS_HIP(&ctx->err, hipEventSynchronize(lease.ev));
    memcpy(out, c.host.p, CountPair::kBytes);
    return WS_OK;
}

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
        (e = hipEventCreate(&ctx->searcher.evk0)) != hipSuccess || (e = hipEventCreate(&ctx->searcher.evk1)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[0].ev_h2d, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[0].ev_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[1].ev_h2d, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->jobs[1].ev_done, hipEventDisableTiming)) != hipSuccess) {
        fail(nullptr, WS_ERR_HIP, "ws_create: %s", hipGetErrorString(e));
        delete ctx;
        return WS_ERR_HIP;
    }
    ctx->num_cus = ctx->searcher.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
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
    for (hipEvent_t e : {ctx->ev0, ctx->ev1, ctx->searcher.evk0, ctx->searcher.evk1, ctx->jobs[0].ev_h2d, ctx->jobs[0].ev_done,
                         ctx->jobs[1].ev_h2d, ctx->jobs[1].ev_done})
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < ws_context::kMaxBands; ++i)
        for (hipEvent_t e : {ctx->ev_band_up[i], ctx->ev_band_done[i], ctx->ev_band_down[i]})
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_mesh)
        if (e) (void)hipEventDestroy(e);
    // every buffer and every lease's event goes with its owner, on this device, with nothing using it.  A batch never
    // waited for: its maps are NOT handed over -- only ws_wait delivers, and a caller who abandoned the batch may have
    // freed the buffers they go to
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
    if (p->view != WS_VIEW_LINEAR && is_census(p->cost)) { // the census match kernel: no marching region, one kernel for the map
        int ow, oh, d0, nd;
        map_dims(p, left, right, &ow, &oh);
        disparity_range(p, left, &d0, &nd);
        out->kernel_kind = 2;
        out->threads = kCtThreads;
        out->tiles = (ow + kCtTile - 1) / kCtTile;
        out->strips = (oh + kCtStrip - 1) / kCtStrip;
        out->strip_rows = kCtStrip;
        out->tile_cols = kCtTile;
        out->d_chunks = (nd + kCtWtaStep - 1) / kCtWtaStep;
        out->lds_bytes = kCtLdsWta;
        return WS_OK;
    }
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
        out->kernel_kind = m.mfma;
    }
    return WS_OK;
}

int ws_search_device(ws_context *ctx, const ws_params *p, const ws_image *left_dev,
                     const ws_image *right_dev, float *out_dev, int out_stride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = check_params(&ctx->err, p, left_dev, right_dev);
    if (rc != WS_OK) return rc;
    if (!out_dev) return fail(&ctx->err, WS_ERR_ARG, "null output");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return search(ctx->searcher, &ctx->err, p, left_dev, right_dev, out_dev, out_stride, nullptr, ctx->status_dev, s);
}

// One boundary call in row bands.  A pixel's result depends on the image rows its window covers and on nothing
// else when smoothFactor == 1 (no raster dependency, no varBlock growth): the map's rows [y0, y1) are the interior
// rows of a search on the sub-images [y0 - half, y1 + half).  So the call is cut into K bands and three queues run
// beside each other: band k+1's image rows go up (copy_stream) while band k is searched (the context's stream) and
// band k-1's map rows come down (down_stream) -- PCIe is full duplex and the copy engines are idle during a search.
// The bytes that cross are the same as in the plain path; only their timing changes.  Results are identical
// (tests/test_gpu_parity.py::test_host_call_in_bands_equals_the_plain_call).
// sp: ws_search_host's spans (both images as whole spans: it checked linear_span; the map dense, out_stride == ow)
static int search_host_banded(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, HostSpan *sp,
                              int wire, int esz, int ow, int oh, int nb)
{
    const int half = (p->block_size - 1) / 2;
    const size_t lb = (size_t)left->width * 3, rb = (size_t)right->width * 3;
    const int H = oh; // (equal heights: the caller checked)
    uint8_t *dl = static_cast<uint8_t *>(ctx->d_left.p), *dr = static_cast<uint8_t *>(ctx->d_right.p);
    float *scratch = static_cast<float *>(ctx->d_out.p);
    HostTrace tr;
    spans_attach(sp, 3);
    tr.mark("attached");
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
            WS_HIP(&ctx->err, span_upload(sp[0], ol, dl + ol, nl, ctx->copy_stream));
            WS_HIP(&ctx->err, span_upload(sp[1], orr, dr + orr, nr, ctx->copy_stream));
            up_to = b;
        }
        tr.mark("up", k);
        WS_HIP(&ctx->err, hipEventRecord(ctx->ev_band_up[k], ctx->copy_stream));
        WS_HIP(&ctx->err, hipStreamWaitEvent(ctx->stream, ctx->ev_band_up[k], 0));
        ws_image bl{dl + (size_t)a * left->stride, left->width, b - a, left->stride};
        ws_image br{dr + (size_t)a * right->stride, right->width, b - a, right->stride};
        float *bout = scratch + (size_t)ow * (a + 2 * half * k); // the band's own map: its border rows are scrap
        int16_t *bout16 = wire == kWireI16 ? static_cast<int16_t *>(ctx->d_out16.p) + (size_t)ow * (a + 2 * half * k) : nullptr;
        if (const int rc = search(ctx->searcher, &ctx->err, p, &bl, &br, bout, ow, bout16, ctx->status_dev, ctx->stream); rc != WS_OK)
            return rc;
        const void *src = wire == kWireI16 ? static_cast<const void *>(bout16 + (size_t)ow * (y0 - a)) : static_cast<const void *>(bout + (size_t)ow * (y0 - a));
        WS_HIP(&ctx->err, hipEventRecord(ctx->ev_band_done[k], ctx->stream));
        WS_HIP(&ctx->err, hipStreamWaitEvent(ctx->down_stream, ctx->ev_band_done[k], 0));
        WS_HIP(&ctx->err, span_download(sp[2], (size_t)ow * y0, (size_t)ow, src, (size_t)ow, (size_t)(y1 - y0), wire, esz, ctx->down_stream));
        WS_HIP(&ctx->err, hipEventRecord(ctx->ev_band_down[k], ctx->down_stream));
        tr.mark("enq", k);
    }
    // a staged map: every band's rows go from the stage to the caller's buffer -- widened on the way -- as soon as they
    // are down, while the bands behind it are still being searched (segment k of the span is band k's download).
    // (Handing a band over earlier, between two later bands' uploads, measured 3 % slower: profiles/r04/host_trace.txt.)
    if (sp[2].down.size() == (size_t)nb) {
        for (int k = 0; k < nb; ++k) {
            WS_HIP(&ctx->err, hipEventSynchronize(ctx->ev_band_down[k]));
            tr.mark("down", k);
            span_scatter_seg(sp[2], sp[2].down[(size_t)k]);
            tr.mark("out", k);
        }
    }
    return WS_OK;
}

int ws_device_status(ws_context *ctx, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    WS_HIP(&ctx->err, hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : ctx->stream));
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

int ws_last_outliers_forms(const ws_context *ctx, ws_outliers_forms *forms)
{
    if (!ctx || !forms) return WS_ERR_ARG;
    for (int i = 0; i < 2; ++i) {
        const OutlierForms &f = ctx->last_outliers_forms[i];
        ws_outliers_pass &o = i == 0 ? forms->integer_pass : forms->double_pass;
        o.row_kernel = f.row_kernel;
        o.row_passes = f.row_passes;
        o.row_per = f.row_per;
        o.col_band = f.col_band;
        o.row_window = f.row_window;
        o.col_window = f.col_window;
    }
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
    int ow, oh, rc = check_params(&ctx->err, p, left, right);
    if (rc == WS_OK) rc = check_out(&ctx->err, p, left, right, out, out_stride, out_dtype, &ow, &oh);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // bands pay when the copies are worth hiding and each band still fills the chip
    // (a census descriptor looks ry rows beyond the window: a band would see "outside the image" there, so a census call
    // is never cut)
    const bool can = (p->view == WS_VIEW_LEFT || p->view == WS_VIEW_RIGHT) && p->smooth_factor == 1.0 && !p->var_block && !is_census(p->cost) &&
                     left->height == right->height && out_stride == ow && linear_span(left) && linear_span(right) &&
                     (size_t)left->stride <= 2 * (size_t)left->width * 3 && (size_t)right->stride <= 2 * (size_t)right->width * 3;
    int nb = ctx->host_bands;
    // (measured on one MI355X, tools/host_bands_time.py: 1.5 Mpixel 0.61 -> 0.47 ms with 2..4 bands,
    // 5.9 Mpixel 2.6 -> 1.5 ms with 5..6; below a megapixel the bands' fixed costs eat the overlap)
    const size_t px = (size_t)ow * oh;
    if (nb < 0) nb = px < ((size_t)1 << 20) ? 0 : px < 3000000 ? 2 : px < 5000000 ? 4 : 6;
    if (!(can && nb >= 2 && oh >= 64 * nb)) nb = 0;
    if (nb && !ctx->down_stream) WS_HIP(&ctx->err, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
    for (int i = 0; i < nb; ++i)
        for (hipEvent_t *e : {&ctx->ev_band_up[i], &ctx->ev_band_done[i], &ctx->ev_band_down[i]})
            if (!*e) WS_HIP(&ctx->err, hipEventCreateWithFlags(e, hipEventDisableTiming));
    // The caller's buffers for the duration of the call (HostSpan): caller-pinned or staged -- every
    // host copy of this library goes the same way, whatever the band setting of the moment, and none through the
    // runtime's pageable path.
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    const int wire = wire_for(p, left, right), esz = out_elem_size(out_dtype);
    const int half = (p->block_size - 1) / 2;
    const size_t map_px = (size_t)ow * (oh + 2 * half * nb); // (in bands: each band's map with its halo rows)
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, map_px * 4)) != WS_OK) return rc;
    if (wire == kWireI16 && (rc = ensure(&ctx->err, ctx->d_out16, map_px * 2)) != WS_OK) return rc;
    span_set(sp[2], out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)oh, &ctx->h_out);
    if (nb) {
        rc = search_host_banded(ctx, p, left, right, sp, wire, esz, ow, oh, nb);
        return call.close(rc, 3, wire, true, "banded host call", {ctx->copy_stream, s, ctx->down_stream});
    }
    spans_attach(sp, 3);
    rc = [&]() -> int {
        if (const int r = call.upload(); r != WS_OK) return r;
        float *dout = static_cast<float *>(ctx->d_out.p);
        int16_t *dout16 = wire == kWireI16 ? static_cast<int16_t *>(ctx->d_out16.p) : nullptr;
        if (const int r = search(ctx->searcher, &ctx->err, p, &call.dl, &call.dr, dout, ow, dout16, ctx->status_dev, s); r != WS_OK) return r;
        const void *src = wire == kWireI16 ? static_cast<const void *>(dout16) : static_cast<const void *>(dout);
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_stride, src, (size_t)ow, (size_t)oh, wire, esz, s));
        return WS_OK;
    }();
    return call.close(rc, 3, wire, true, "host call");
}

// The batched host path keeps two pairs in flight: while one is searched (context stream) the next
// one's images go up and the previous one's map comes down on a second stream, straight from / to
// the caller's buffers as linear copies (see ws_search_host).
static int flush_job(ws_context *ctx, Job &j)
{
    if (!j.pending) return WS_OK;
    j.pending = false;
    WS_HIP(&ctx->err, hipStreamWaitEvent(ctx->copy_stream, j.ev_done, 0));
    const int esz = out_elem_size(j.dtype);
    const size_t first = (size_t)j.row0 * j.w;
    const void *src = j.wire == kWireI16 ? static_cast<const void *>(static_cast<const int16_t *>(j.out16.p) + first)
                                         : static_cast<const void *>(static_cast<const float *>(j.out.p) + first);
    WS_HIP(&ctx->err, span_download(ctx->batch_spans[(size_t)j.out_span], 0, (size_t)j.out_stride, src, (size_t)j.w, (size_t)j.h, j.wire, esz,
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
    int ow, oh, rc = check_params(&ctx->err, p, left, right);
    if (rc == WS_OK) rc = check_out(&ctx->err, p, left, right, out, out_stride, out_dtype, &ow, &oh);
    if (rc != WS_OK) return rc;
    if (map_rows < 0) {
        map_row0 = 0;
        map_rows = oh;
    }
    if (map_row0 < 0 || map_rows < 1 || map_row0 + map_rows > oh)
        return fail(&ctx->err, WS_ERR_ARG, "map rows [%d, %d) outside [0, %d)", map_row0, map_row0 + map_rows, oh);
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    Job &job = ctx->jobs[ctx->job_next];
    Job &prev = ctx->jobs[ctx->job_next ^ 1];
    if ((rc = flush_job(ctx, job)) != WS_OK) return rc; // (only after an error left it pending)
    // this slot's previous pair: a map that came down through the slot's stage goes to its caller now, before the
    // stage is used again
    if (job.out_span >= 0 && !ctx->batch_spans[(size_t)job.out_span].down.empty()) {
        WS_HIP(&ctx->err, hipStreamSynchronize(ctx->copy_stream));
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
    if ((rc = ensure(&ctx->err, job.in, off_r + span_r)) != WS_OK || (rc = ensure(&ctx->err, job.out, out_elems * 4)) != WS_OK ||
        (rc = ensure(&ctx->err, job.out16, out_elems * 2)) != WS_OK)
        return rc;
    uint8_t *d_left = static_cast<uint8_t *>(job.in.p), *d_right = d_left + off_r;
    hipStream_t cs = ctx->copy_stream;
    const int esz = out_elem_size(out_dtype);
    span_set(sp[2], out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)map_rows, &job.h_out);
    spans_attach(sp, 3);
    const size_t first = ctx->batch_spans.size();
    for (int i = 0; i < 3; ++i) ctx->batch_spans.push_back(sp[i]);
    HostSpan *bs = ctx->batch_spans.data() + first; // (valid until the next push_back: only used inside this call)
    job.out_span = (int)first + 2;
    // bytes that cross through this slot's pinned buffers (gathered cut-outs, stages): the slot's previous upload from
    // them must be through
    if (bs[0].how != HostSpan::kCallerPinned || bs[1].how != HostSpan::kCallerPinned) WS_HIP(&ctx->err, hipEventSynchronize(job.ev_h2d));
    ws_image dl, dr;
    WS_HIP(&ctx->err, upload_image(bs[0], left, d_left, cs, &dl));
    WS_HIP(&ctx->err, upload_image(bs[1], right, d_right, cs, &dr));
    WS_HIP(&ctx->err, hipEventRecord(job.ev_h2d, cs));
    WS_HIP(&ctx->err, hipStreamWaitEvent(ctx->stream, job.ev_h2d, 0));
    job.wire = wire_for(p, left, right);
    int16_t *out16 = job.wire == kWireI16 ? static_cast<int16_t *>(job.out16.p) : nullptr;
    if ((rc = search(ctx->searcher, &ctx->err, p, &dl, &dr, static_cast<float *>(job.out.p), ow, out16, ctx->status_dev, ctx->stream)) != WS_OK)
        return rc;
    WS_HIP(&ctx->err, hipEventRecord(job.ev_done, ctx->stream));
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
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
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
        return fail(&ctx->err, WS_ERR_ARG, "bad warp arguments");
    double inv[9];
    if (!invert3x3(m, inv)) return fail(&ctx->err, WS_ERR_ARG, "singular warp matrix");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    WS_HIP(&ctx->err, launch_warp(src_dev, src_w, src_h, src_stride, dst_dev, dst_w, dst_h, dst_stride, inv, s));
    return WS_OK;
}

int ws_warp_nearest_host(ws_context *ctx, const double *src, int src_w, int src_h, int src_stride,
                         const double m[9], double *dst, int dst_w, int dst_h, int dst_stride)
{
    if (!ctx) return WS_ERR_ARG;
    if (!src || !dst || !m || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 || src_stride < src_w ||
        dst_stride < dst_w)
        return fail(&ctx->err, WS_ERR_ARG, "bad warp arguments");
    // disparity maps are integer valued (or f32 sub-pixel): f32 on the device, CV_64F at the boundary; the floats
    // cross from / to pinned memory of the library's own
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    const size_t ns = (size_t)src_w * src_h, nd = (size_t)dst_w * dst_h;
    WS_HIP(&ctx->err, host_ensure(ctx->h_left, ns * 4));
    WS_HIP(&ctx->err, host_ensure(ctx->h_right, nd * 4));
    float *hs = reinterpret_cast<float *>(ctx->h_left.p), *hd = reinterpret_cast<float *>(ctx->h_right.p);
    for (int y = 0; y < src_h; ++y)
        for (int x = 0; x < src_w; ++x) hs[(size_t)y * src_w + x] = (float)src[(size_t)y * src_stride + x];
    int rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, ns * 4)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out64, nd * 4)) != WS_OK) return rc;
    WS_HIP(&ctx->err, hipMemcpyAsync(ctx->d_out.p, hs, ns * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = ws_warp_nearest_device(ctx, static_cast<const float *>(ctx->d_out.p), src_w, src_h, src_w, m,
                                static_cast<float *>(ctx->d_out64.p), dst_w, dst_h, dst_w, ctx->stream);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipMemcpyAsync(hd, ctx->d_out64.p, nd * 4, hipMemcpyDeviceToHost, ctx->stream));
    WS_HIP(&ctx->err, hipStreamSynchronize(ctx->stream));
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
        return fail(&ctx->err, WS_ERR_ARG, "bad rectify arguments");
    double inv[9];
    if (!invert3x3(H, inv)) return fail(&ctx->err, WS_ERR_ARG, "singular warp matrix");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    WS_HIP(&ctx->err, launch_rectify(src_dev->data, src_dev->width, src_dev->height, src_dev->stride, inv, dst_dev, dst_w, dst_h,
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
    if (!p || !image_ok(left) || !image_ok(right) || !H || !Hp) return fail(&ctx->err, WS_ERR_ARG, "null or malformed image / params / homography");
    if (p->view == WS_VIEW_LINEAR) return fail(&ctx->err, WS_ERR_ARG, "ImageRectifier has no LinearSearch method");
    int ow, oh, lw, lh, rw, rh; // the map in the original frame; the rectified images
    int rc = check_out(&ctx->err, p, left, right, out, out_stride, out_dtype, &ow, &oh);
    if (rc != WS_OK) return rc;
    double h_inv[9], hp_inv[9], back[9]; // M^-1 of the two forward warps; M^-1 of the warp back, M = H_.inv()
    if (!invert3x3(H, h_inv) || !invert3x3(Hp, hp_inv) || !invert3x3(h_inv, back)) return fail(&ctx->err, WS_ERR_ARG, "singular homography");
    if ((rc = ws_rectified_size(H, left->width, left->height, &lw, &lh)) != WS_OK ||
        (rc = ws_rectified_size(Hp, right->width, right->height, &rw, &rh)) != WS_OK)
        return fail(&ctx->err, rc, "%s", ws_last_error(nullptr));
    const ws_image shape_l{left->data, lw, lh, 3 * lw}, shape_r{right->data, rw, rh, 3 * rw};
    if ((rc = check_params(&ctx->err, p, &shape_l, &shape_r)) != WS_OK) return rc;
    int mw, mh; // the rectified map
    map_dims(p, &shape_l, &shape_r, &mw, &mh);
    if ((rect_left && rect_left_stride < 3 * lw) || (rect_right && rect_right_stride < 3 * rw))
        return fail(&ctx->err, WS_ERR_ARG, "rectified image stride below 3 * width");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_rect_left, (size_t)lw * lh * 3)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_rect_right, (size_t)rw * rh * 3)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, (size_t)mw * mh * 4)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out64, (size_t)ow * oh * 4)) != WS_OK) return rc;
    const int esz = out_elem_size(out_dtype);
    span_set(sp[2], out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)oh, &ctx->h_out);
    if (rect_left) span_set(sp[3], rect_left, (size_t)rect_left_stride, 3 * (size_t)lw, (size_t)lh, &ctx->h_aux[0]);
    if (rect_right) span_set(sp[4], rect_right, (size_t)rect_right_stride, 3 * (size_t)rw, (size_t)rh, &ctx->h_aux[1]);
    spans_attach(sp, 5);
    uint8_t *drl = static_cast<uint8_t *>(ctx->d_rect_left.p), *drr = static_cast<uint8_t *>(ctx->d_rect_right.p);
    rc = [&]() -> int {
        if (const int r = call.upload(); r != WS_OK) return r;
        const ws_image &dl = call.dl, &dr = call.dr;
        // warpPerspective(leftImage_, .., H_, size), warpPerspective(rightImage_, .., Hp_, size) (rectification.cpp:486-493)
        WS_HIP(&ctx->err, launch_rectify(dl.data, dl.width, dl.height, dl.stride, h_inv, drl, lw, lh, 3 * lw, s));
        WS_HIP(&ctx->err, launch_rectify(dr.data, dr.width, dr.height, dr.stride, hp_inv, drr, rw, rh, 3 * rw, s));
        // BlockSearch on the rectified pair (rectification.cpp:67-68, :79-80)
        const ws_image il{drl, lw, lh, 3 * lw}, ir{drr, rw, rh, 3 * rw};
        float *rect_map = static_cast<float *>(ctx->d_out.p), *map = static_cast<float *>(ctx->d_out64.p);
        if (const int rc2 = search(ctx->searcher, &ctx->err, p, &il, &ir, rect_map, mw, nullptr, ctx->status_dev, s); rc2 != WS_OK) return rc2;
        // cv::warpPerspective(disparityMap_rect, .., H_.inv(), original size, INTER_NEAREST) (rectification.cpp:70-75, :82-87)
        WS_HIP(&ctx->err, launch_warp(rect_map, mw, mh, mw, map, ow, oh, ow, back, s));
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_stride, map, (size_t)ow, (size_t)oh, kWireF32, esz, s));
        if (rect_left) WS_HIP(&ctx->err, span_download_bytes(sp[3], 0, (size_t)rect_left_stride, drl, 3 * (size_t)lw, (size_t)lh, s));
        if (rect_right) WS_HIP(&ctx->err, span_download_bytes(sp[4], 0, (size_t)rect_right_stride, drr, 3 * (size_t)rw, (size_t)rh, s));
        return WS_OK;
    }();
    return call.close(rc, 5, -1, true, "unrectified host call"); // (this call has never reported its paths)
}

// ---- consumers of the map (src/Reconstruction/reconstruction.cpp) ----------------------

int ws_remove_disparity_outliers(ws_context *ctx, float *map, int width, int height, int stride, int kernel_size,
                                 float thr_front, float thr_back)
{
    if (!ctx) return WS_ERR_ARG;
    if (!map || width <= 0 || height <= 0 || stride < width || kernel_size < 1)
        return fail(&ctx->err, WS_ERR_ARG, "bad removeDisparityOutliers arguments");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    int rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, n * 4)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out64, std::max(n * 8, outliers_u32_scratch_bytes(width, height, ctx->num_cus)))) != WS_OK) return rc;
    if (!ctx->d_flag.p) {
        if ((rc = ensure(&ctx->err, ctx->d_flag, 256)) != WS_OK) return rc;
        WS_HIP(&ctx->err, hipMemsetAsync(ctx->d_flag.p, 0, 256, s));
    }
    float *dmap = static_cast<float *>(ctx->d_out.p);
    // the caller's map for the duration of the call (HostSpan, like ws_search_host: no pageable copies)
    HostSpan sp[1];
    span_set(sp[0], map, (size_t)stride * 4, (size_t)width * 4, (size_t)height, &ctx->h_out);
    spans_attach(sp, 1);
    // 8-bit maps (the pipeline's PNG: integers in [0, 255]) take the 32-bit integer kernels; a map with any other value
    // raises status word 1, is left as uploaded, and goes through the double kernels after the first synchronisation
    const bool try_u32 = ctx->d_flag.p && outliers_u32_applies(width, height, kernel_size, ctx->num_cus);
    ctx->last_outliers_forms[0] = ctx->last_outliers_forms[1] = OutlierForms{};
    auto pass = [&](bool u32) -> int { // the kernels on the uploaded map, the result down to the caller's
        if (u32)
            WS_HIP(&ctx->err, launch_outliers_u32(dmap, width, width, height, kernel_size, thr_front, thr_back, static_cast<uint32_t *>(ctx->d_out64.p),
                                            static_cast<uint32_t *>(ctx->d_flag.p), ctx->status_dev + 1, ctx->num_cus, s,
                                            &ctx->last_outliers_forms[0]));
        else
            WS_HIP(&ctx->err, launch_outliers(dmap, width, width, height, kernel_size, thr_front, thr_back, static_cast<double *>(ctx->d_out64.p), s,
                                        &ctx->last_outliers_forms[1]));
        WS_HIP(&ctx->err, span_download_bytes(sp[0], 0, (size_t)stride * 4, dmap, (size_t)width * 4, (size_t)height, s));
        return WS_OK;
    };
    rc = [&]() -> int {
        WS_HIP(&ctx->err, span_upload_rows(sp[0], 0, (size_t)stride * 4, dmap, (size_t)width * 4, (size_t)height, s));
        return pass(try_u32);
    }();
    const hipError_t es = hipStreamSynchronize(s);
    ctx->last_outliers_path = try_u32 ? 1 : 0;
    if (rc == WS_OK && es != hipSuccess) rc = fail(&ctx->err, WS_ERR_HIP, "removeDisparityOutliers: %s", hipGetErrorString(es));
    if (rc != WS_OK || !try_u32 || !ctx->status_host[1]) return finish_host_call(ctx, rc, sp, 1, {}, "removeDisparityOutliers");
    ctx->status_host[1] = 0;
    ctx->last_outliers_path = 2;
    rc = [&]() -> int {
        WS_HIP(&ctx->err, hipMemsetAsync(ctx->d_flag.p, 0, 256, s));
        return pass(false);
    }();
    return finish_host_call(ctx, rc, sp, 1, {s}, "removeDisparityOutliers");
}

static int depth_vertices_host(ws_context *ctx, const float *in, int width, int height, int stride, int input_is_depth,
                               float focal, float baseline, const float *k, const ws_image *bgr, float *depth,
                               int depth_stride, float *positions, uint8_t *colors)
{
    if (!ctx) return WS_ERR_ARG;
    if (!in || width <= 0 || height <= 0 || stride < width) return fail(&ctx->err, WS_ERR_ARG, "bad map");
    if (positions && (!colors || !k || !bgr || !bgr->data || bgr->width != width || bgr->height != height ||
                      bgr->stride < 3 * width))
        return fail(&ctx->err, WS_ERR_ARG, "back-projection needs K, a colour image of the map's size and both outputs");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    int rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, n * 4)) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out64, n * 4 + n * 16 + n * 4)) != WS_OK) return rc;
    // the caller's buffers for the duration of the call (HostSpan, like ws_search_host: no pageable copies)
    HostSpan sp[5];
    if (positions && (rc = ensure(&ctx->err, ctx->d_left, image_span(sp[4], bgr, &ctx->h_left))) != WS_OK) return rc;
    float *din = static_cast<float *>(ctx->d_out.p);
    uint8_t *base = static_cast<uint8_t *>(ctx->d_out64.p);
    float *dpos = reinterpret_cast<float *>(base);           // n * 16 bytes, 16-byte aligned
    float *ddepth = reinterpret_cast<float *>(base + n * 16); // n * 4
    uint8_t *dcol = base + n * 20;                            // n * 4
    span_set(sp[0], in, (size_t)stride * 4, (size_t)width * 4, (size_t)height, &ctx->h_out);
    if (depth) span_set(sp[1], depth, (size_t)depth_stride * 4, (size_t)width * 4, (size_t)height, &ctx->h_right);
    if (positions) span_set(sp[2], positions, n * 16, n * 16, 1, &ctx->h_aux[0]);
    if (positions) span_set(sp[3], colors, n * 4, n * 4, 1, &ctx->h_aux[1]);
    spans_attach(sp, 5);
    rc = [&]() -> int {
        WS_HIP(&ctx->err, span_upload_rows(sp[0], 0, (size_t)stride * 4, din, (size_t)width * 4, (size_t)height, s));
        ws_image dbgr{static_cast<const uint8_t *>(ctx->d_left.p), width, height, width * 3};
        if (positions) WS_HIP(&ctx->err, upload_image(sp[4], bgr, static_cast<uint8_t *>(ctx->d_left.p), s, &dbgr));
        WS_HIP(&ctx->err, launch_depth_vertices(din, width, width, height, focal, baseline, k, dbgr.data, dbgr.stride, depth ? ddepth : nullptr, width,
                                          positions ? dpos : nullptr, positions ? dcol : nullptr, input_is_depth, s));
        if (depth) WS_HIP(&ctx->err, span_download_bytes(sp[1], 0, (size_t)depth_stride * 4, ddepth, (size_t)width * 4, (size_t)height, s));
        if (positions) {
            WS_HIP(&ctx->err, span_download_bytes(sp[2], 0, n * 16, dpos, n * 16, 1, s));
            WS_HIP(&ctx->err, span_download_bytes(sp[3], 0, n * 4, dcol, n * 4, 1, s));
        }
        return WS_OK;
    }();
    return finish_host_call(ctx, rc, sp, 5, {s}, "depth / vertices");
}

int ws_convert_disparity_to_depth(ws_context *ctx, const float *disp, int width, int height, int stride, float focal_length,
                                  float baseline, float *depth, int depth_stride)
{
    if (!depth || depth_stride < width) return ctx ? fail(&ctx->err, WS_ERR_ARG, "bad depth output") : WS_ERR_ARG;
    return depth_vertices_host(ctx, disp, width, height, stride, 0, focal_length, baseline, nullptr, nullptr, depth,
                               depth_stride, nullptr, nullptr);
}

int ws_back_project(ws_context *ctx, const float *depth, int width, int height, int stride, const float intrinsics[9],
                    const ws_image *bgr, float *positions, uint8_t *colors)
{
    if (!positions || !colors) return ctx ? fail(&ctx->err, WS_ERR_ARG, "null vertex output") : WS_ERR_ARG;
    return depth_vertices_host(ctx, depth, width, height, stride, 1, 0.0f, 0.0f, intrinsics, bgr, nullptr, 0, positions, colors);
}

// ---- WriteMesh (reconstruction.cpp:72-149) on the device: the kernels of ws_mesh.hip lay out the file's text, the host
// only moves the finished bytes into the file ------------------------------------------------------------------------

static constexpr size_t kMeshChunk = 8u << 20; // the text comes down in chunks of this size: pinned memory stays 2 chunks

static int mesh_args(ws_context *ctx, const void *pos, const void *col, int width, int height, const char *path)
{
    if (!path) return fail(&ctx->err, WS_ERR_ARG, "null mesh path");
    if (!pos || !col) return fail(&ctx->err, WS_ERR_ARG, "null input buffer");
    if (width <= 0 || height <= 0) return fail(&ctx->err, WS_ERR_ARG, "bad mesh size %d x %d", width, height);
    if ((uint64_t)width * (uint64_t)height > UINT32_MAX)
        return fail(&ctx->err, WS_ERR_ARG, "a %d x %d mesh has more vertices than 32-bit indices reach", width, height);
    return WS_OK;
}

static FILE *mesh_open(ws_context *ctx, const char *path, int *rc)
{
    FILE *f = fopen(path, "wb");
    *rc = f ? WS_OK : fail(&ctx->err, WS_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    return f;
}

// The end of a mesh call: the stream idle (a failed call may have copies in flight into the chunks), the file closed.
static int mesh_close(ws_context *ctx, int rc, FILE *f, hipStream_t s)
{
    if (rc != WS_OK) (void)hipStreamSynchronize(s);
    if (fclose(f) != 0 && rc == WS_OK) rc = fail(&ctx->err, WS_ERR_IO, "closing the mesh file failed: %s", strerror(errno));
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
    if ((rc = ensure(&ctx->err, ctx->d_mesh, 64 + nb * 16)) != WS_OK) return rc;
    for (HostBuf &b : ctx->h_mesh) WS_HIP(&ctx->err, host_ensure(b, kMeshChunk));
    for (hipEvent_t &e : ctx->ev_mesh)
        if (!e) WS_HIP(&ctx->err, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint8_t *base = static_cast<uint8_t *>(ctx->d_mesh.p);
    auto *meta = reinterpret_cast<unsigned long long *>(base);             // {header bytes, file bytes, faces}
    auto *sums = reinterpret_cast<uint32_t *>(base + 64);                  // 2 words per workgroup
    auto *offs = reinterpret_cast<unsigned long long *>(base + 64 + nb * 8); // 1 word per workgroup
    WS_HIP(&ctx->err, launch_mesh_count(dpos, dcol, w, h, thr, sums, offs, meta, s));
    WS_HIP(&ctx->err, hipMemcpyAsync(ctx->h_mesh[0].p, meta, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    WS_HIP(&ctx->err, hipStreamSynchronize(s));
    unsigned long long hm[3];
    memcpy(hm, ctx->h_mesh[0].p, sizeof hm);
    tr.mark("sized");
    const size_t bytes = (size_t)hm[1];
    if ((rc = ensure(&ctx->err, ctx->d_mesh_text, bytes)) != WS_OK) return rc;
    const char *text = static_cast<const char *>(ctx->d_mesh_text.p);
    WS_HIP(&ctx->err, launch_mesh_write(dpos, dcol, w, h, thr, offs, meta, static_cast<char *>(ctx->d_mesh_text.p), s));
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
            WS_HIP(&ctx->err, hipMemcpyAsync(ctx->h_mesh[cur].p, text + off, len, hipMemcpyDeviceToHost, s));
            WS_HIP(&ctx->err, hipEventRecord(ctx->ev_mesh[cur], s));
            off += len;
        }
        if (pending >= 0) {
            const auto t0 = now();
            WS_HIP(&ctx->err, hipEventSynchronize(ctx->ev_mesh[pending]));
            const auto t1 = now();
            if (fwrite(ctx->h_mesh[pending].p, 1, pending_len, f) != pending_len)
                return fail(&ctx->err, WS_ERR_IO, "writing the mesh file failed: %s", strerror(errno));
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
        return fail(&ctx->err, WS_ERR_ARG, "positions must be 16-byte aligned, colors 4-byte aligned");
    FILE *f = mesh_open(ctx, path, &rc);
    if (!f) return rc;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    rc = [&]() -> int {
        WS_HIP(&ctx->err, hipSetDevice(ctx->device));
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
    if (stride < width) return fail(&ctx->err, WS_ERR_ARG, "bad depth stride");
    if (!intrinsics || !bgr->data || bgr->width != width || bgr->height != height || bgr->stride < 3 * width)
        return fail(&ctx->err, WS_ERR_ARG, "reconstruction needs K and a colour image of the depth map's size");
    FILE *f = mesh_open(ctx, path, &rc);
    if (!f) return rc;
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)width * height;
    // as ws_back_project, without the vertices' way down: depth and image go up (HostSpan), the vertices stay on the device
    HostSpan sp[2];
    rc = [&]() -> int {
        WS_HIP(&ctx->err, hipSetDevice(ctx->device));
        int r;
        if ((r = ensure(&ctx->err, ctx->d_out, n * 4)) != WS_OK) return r;
        if ((r = ensure(&ctx->err, ctx->d_out64, n * 20)) != WS_OK) return r;
        return ensure(&ctx->err, ctx->d_left, image_span(sp[1], bgr, &ctx->h_left));
    }();
    if (rc != WS_OK) return mesh_close(ctx, rc, f, s);
    float *din = static_cast<float *>(ctx->d_out.p);
    uint8_t *vbase = static_cast<uint8_t *>(ctx->d_out64.p);
    float *dpos = reinterpret_cast<float *>(vbase); // n * 16 bytes, 16-byte aligned
    uint8_t *dcol = vbase + n * 16;                 // n * 4
    span_set(sp[0], depth, (size_t)stride * 4, (size_t)width * 4, (size_t)height, &ctx->h_out);
    spans_attach(sp, 2);
    rc = [&]() -> int {
        WS_HIP(&ctx->err, span_upload_rows(sp[0], 0, (size_t)stride * 4, din, (size_t)width * 4, (size_t)height, s));
        ws_image dbgr{static_cast<const uint8_t *>(ctx->d_left.p), width, height, width * 3};
        WS_HIP(&ctx->err, upload_image(sp[1], bgr, static_cast<uint8_t *>(ctx->d_left.p), s, &dbgr));
        WS_HIP(&ctx->err, launch_depth_vertices(din, width, width, height, 0.0f, 0.0f, intrinsics, dbgr.data, dbgr.stride, nullptr, width,
                                          dpos, dcol, 1, s));
        return mesh_to_file(ctx, dpos, dcol, width, height, edge_threshold, f, s);
    }();
    rc = finish_host_call(ctx, rc, sp, 2, {s}, "reconstruction");
    return mesh_close(ctx, rc, f, s);
}

// ---- the census transform on its own (the searches run it on the Searcher's planes) --------------------------------

static int census_transform_args(std::string *err, const ws_image *img, int cost, const void *out, int out_stride)
{
    if (!image_ok(img)) return fail(err, WS_ERR_ARG, "null or malformed image");
    if (!is_census(cost)) return fail(err, WS_ERR_ARG, "cost %d is not a census cost", cost);
    if (!out) return fail(err, WS_ERR_ARG, "null output");
    if (out_stride < img->width) return fail(err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, img->width);
    return WS_OK;
}

int ws_census_transform_device(ws_context *ctx, const ws_image *img_dev, int cost, uint64_t *out_dev, int out_stride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    if (const int rc = census_transform_args(&ctx->err, img_dev, cost, out_dev, out_stride); rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    WS_HIP(&ctx->err, launch_census_transform(img_dev->data, img_dev->width, img_dev->height, img_dev->stride, cost, out_dev, out_stride, true, s));
    return WS_OK;
}

int ws_census_transform_host(ws_context *ctx, const ws_image *img, int cost, uint64_t *out, int out_stride)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = census_transform_args(&ctx->err, img, cost, out, out_stride);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t w = (size_t)img->width, h = (size_t)img->height;
    HostSpan sp[2];
    if ((rc = ensure(&ctx->err, ctx->d_left, image_span(sp[0], img, &ctx->h_left))) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out64, w * h * 8)) != WS_OK) return rc;
    span_set(sp[1], out, (size_t)out_stride * 8, w * 8, h, &ctx->h_out);
    spans_attach(sp, 2);
    rc = [&]() -> int {
        ws_image di;
        WS_HIP(&ctx->err, upload_image(sp[0], img, static_cast<uint8_t *>(ctx->d_left.p), s, &di));
        WS_HIP(&ctx->err, launch_census_transform(di.data, di.width, di.height, di.stride, cost, ctx->d_out64.p, di.width, true, s));
        WS_HIP(&ctx->err, span_download_bytes(sp[1], 0, (size_t)out_stride * 8, ctx->d_out64.p, w * 8, h, s));
        return WS_OK;
    }();
    return finish_host_call(ctx, rc, sp, 2, {s}, "census transform");
}

int ws_timer_begin(ws_context *ctx, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    WS_HIP(&ctx->err, hipEventRecord(ctx->ev0, stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    return WS_OK;
}

int ws_timer_end(ws_context *ctx, void *stream, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return WS_ERR_ARG;
    WS_HIP(&ctx->err, hipEventRecord(ctx->ev1, stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    WS_HIP(&ctx->err, hipEventSynchronize(ctx->ev1));
    WS_HIP(&ctx->err, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return WS_OK;
}

int ws_set_profiling(ws_context *ctx, int enable)
{
    if (!ctx) return WS_ERR_ARG;
    ctx->searcher.profiling = enable != 0;
    ctx->searcher.kernel_timed = false;
    return WS_OK;
}

int ws_last_kernel_ms(ws_context *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return WS_ERR_ARG;
    if (!ctx->searcher.kernel_timed) return fail(&ctx->err, WS_ERR_ARG, "no marching-kernel launch was timed (ws_set_profiling off, or the generic path ran)");
    WS_HIP(&ctx->err, hipEventSynchronize(ctx->searcher.evk1));
    WS_HIP(&ctx->err, hipEventElapsedTime(elapsed_ms, ctx->searcher.evk0, ctx->searcher.evk1));
    return WS_OK;
}

int ws_last_max_block(ws_context *ctx, int block_size, int *max_block)
{
    if (!ctx || !max_block) return WS_ERR_ARG;
    *max_block = block_size;
    if (!ctx->searcher.var_block_ran) return WS_OK;
    int v = 0;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    WS_HIP(&ctx->err, hipDeviceSynchronize());
    WS_HIP(&ctx->err, hipMemcpy(&v, ctx->searcher.max_block.p, sizeof v, hipMemcpyDeviceToHost));
    if (v > block_size) *max_block = v;
    return WS_OK;
}

int ws_last_launch_info(const ws_context *ctx, char *kernel_name, int name_cap, int *threads,
                        int *workgroups, int *lds_bytes)
{
    if (!ctx) return WS_ERR_ARG;
    if (kernel_name && name_cap > 0) {
        strncpy(kernel_name, ctx->searcher.last_kernel.c_str(), (size_t)name_cap - 1);
        kernel_name[name_cap - 1] = 0;
    }
    if (threads) *threads = ctx->searcher.last_threads;
    if (workgroups) *workgroups = ctx->searcher.last_wgs;
    if (lds_bytes) *lds_bytes = ctx->searcher.last_lds;
    return WS_OK;
}

int ws_set_tuning(ws_context *ctx, int x_runs_per_tile, int strip_rows, int threads)
{
    if (!ctx || x_runs_per_tile < 0 || strip_rows < 0 || threads < 0) return WS_ERR_ARG;
    ctx->searcher.tune[0] = x_runs_per_tile;
    ctx->searcher.tune[1] = strip_rows;
    ctx->searcher.tune[2] = threads;
    return WS_OK;
}

} // extern "C"
