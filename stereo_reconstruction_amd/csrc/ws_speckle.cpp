// ws_speckle.cpp -- the speckle filter of include/ws_stereo.h (extension): argument checks, the context's scratch for it
// (SpeckleState) under its lease, the launches of ws_speckle.hip, on device memory or on the caller's host map (through
// ws_staging.h).
#include "ws_context.h"

#include <math.h>

namespace wsamd {
namespace {

// Rule 6 of the header, before anything else: with a null context the refusal is still named (ws_last_error(NULL)).
int check_speckle(std::string *err, const float *map, int w, int h, int stride, const ws_speckle_params *sp)
{
    if (!sp) return fail(err, WS_ERR_ARG, "null ws_speckle_params");
    if (isnan(sp->new_val)) return fail(err, WS_ERR_ARG, "new_val is NaN");
    if (!(sp->max_diff >= 0.0f)) return fail(err, WS_ERR_ARG, "max_diff %g: must be >= 0 (not NaN)", (double)sp->max_diff);
    if (sp->max_speckle_size < 0) return fail(err, WS_ERR_ARG, "max_speckle_size %d: must be >= 0", sp->max_speckle_size);
    if (!map) return fail(err, WS_ERR_ARG, "null map");
    if (w < 1 || h < 1 || stride < w) return fail(err, WS_ERR_ARG, "bad map size or stride (%d x %d, stride %d)", w, h, stride);
    if ((long long)w * h >= (1LL << 31)) return fail(err, WS_ERR_ARG, "map of %d x %d: w * h must be below 2^31", w, h);
    return WS_OK;
}

int check_call(ws_context *ctx, const float *map, int w, int h, int stride, const ws_speckle_params *sp)
{
    if (const int rc = check_speckle(ctx ? &ctx->err : nullptr, map, w, h, stride, sp); rc != WS_OK) return rc;
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    return WS_OK;
}

// Zeroed counters, the four kernels, and the counts on their way to the host -- all on s.
int filter_on(ws_context *ctx, float *map, int w, int h, int stride, const ws_speckle_params *sp, hipStream_t s)
{
    SpeckleState &S = ctx->speckle;
    int rc;
    const size_t n = (size_t)w * h;
    const size_t slot_bytes = speckle_slot_words() * sizeof(unsigned long long);
    if ((rc = ensure(&ctx->err, S.planes, 4 * n * sizeof(int))) != WS_OK) return rc;
    if ((rc = S.counts.reserve(&ctx->err, slot_bytes)) != WS_OK) return rc;
    SpeckleArgs a{};
    a.map = map;
    a.w = w;
    a.h = h;
    a.stride = stride;
    a.new_val = sp->new_val;
    a.max_diff = sp->max_diff;
    a.max_size = sp->max_speckle_size;
    a.label = static_cast<int *>(S.planes.p);
    a.parent = a.label + n;
    a.count = a.parent + n;
    a.local = a.count + n;
    auto *slots = static_cast<unsigned long long *>(S.counts.dev.p), *counts = slots + speckle_slot_words();
    WS_HIP(&ctx->err, hipMemsetAsync(slots, 0, slot_bytes, s));
    WS_HIP(&ctx->err, launch_speckle(a, slots, counts, s));
    return S.counts.fetch(&ctx->err, counts, s);
}

// ... under the filter's lease
int enqueue_filter(ws_context *ctx, float *map, int w, int h, int stride, const ws_speckle_params *sp, hipStream_t s)
{
    ScratchLease &lease = ctx->speckle.lease;
    if (const int rc = lease.begin(&ctx->err, s); rc != WS_OK) return rc;
    return lease.end(&ctx->err, s, filter_on(ctx, map, w, h, stride, sp, s));
}

} // namespace
} // namespace wsamd

using namespace wsamd;

extern "C" {

int ws_filter_speckles_device(ws_context *ctx, float *map_dev, int w, int h, int stride, const ws_speckle_params *sp,
                              void *stream)
{
    int rc = check_call(ctx, map_dev, w, h, stride, sp);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return enqueue_filter(ctx, map_dev, w, h, stride, sp, s);
}

// The map goes up (dense), is filtered on the context's stream and comes back down into the caller's rows; the row
// padding is never written.  One synchronisation at the end.
int ws_filter_speckles_host(ws_context *ctx, float *map, int w, int h, int stride, const ws_speckle_params *sp)
{
    int rc = check_call(ctx, map, w, h, stride, sp);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if ((rc = ensure(&ctx->err, ctx->d_out, (size_t)w * h * sizeof(float))) != WS_OK) return rc;
    float *dmap = static_cast<float *>(ctx->d_out.p);
    // the caller's map for the duration of the call (HostSpan, like ws_search_host)
    HostSpan sp1[1];
    span_set(sp1[0], map, (size_t)stride * 4, (size_t)w * 4, (size_t)h, &ctx->h_out);
    spans_attach(sp1, 1);
    rc = [&]() -> int {
        WS_HIP(&ctx->err, span_upload_rows(sp1[0], 0, (size_t)stride * 4, dmap, (size_t)w * 4, (size_t)h, s));
        if (const int r = enqueue_filter(ctx, dmap, w, h, w, sp, s); r != WS_OK) return r;
        WS_HIP(&ctx->err, span_download_bytes(sp1[0], 0, (size_t)stride * 4, dmap, (size_t)w * 4, (size_t)h, s));
        return WS_OK;
    }();
    return finish_host_call(ctx, rc, sp1, 1, {s}, "speckle filter host call");
}

int ws_last_speckle_counts(ws_context *ctx, unsigned long long counts[2])
{
    if (!ctx || !counts) return WS_ERR_ARG;
    return read_counts(ctx, ctx->speckle.counts, ctx->speckle.lease, "no speckle filter has run on this context", counts);
}

} // extern "C"
