// ws_lr.cpp -- the left-right consistency check of include/ws_stereo.h (extension): argument checks, the context's
// scratch for it (LrState), the launches of ws_lr.hip, and the calls that first search both views of a pair with the
// search dispatch (ws_search.h), on device memory or on the caller's host buffers (through ws_staging.h).
#include "ws_context.h"

#include <stdint.h>

namespace wsamd {

int check_lr(std::string *err, const ws_lr_params *lr)
{
    if (!lr) return fail(err, WS_ERR_ARG, "null ws_lr_params");
    if (!(lr->max_diff >= 0.0f)) return fail(err, WS_ERR_ARG, "max_diff %g: must be >= 0 (not NaN)", (double)lr->max_diff);
    if (lr->fill != WS_LR_FILL_NONE && lr->fill != WS_LR_FILL_BACKGROUND) return fail(err, WS_ERR_ARG, "unknown fill %d", lr->fill);
    return WS_OK;
}

namespace {

// the bytes a map of h rows of w floats, `stride` floats apart, occupies
Extent map_extent(const float *p, int w, int h, int stride) { return Extent(p, (size_t)stride * 4, (size_t)w * 4, (size_t)h); }

// p run as the left view and as the right view, each checked as ws_search_host checks it, the left view first
int view_params(std::string *err, const ws_params *p, const ws_image *L, const ws_image *R, ws_params q[2])
{
    if (!p) return fail(err, WS_ERR_ARG, "null or malformed image / params");
    for (int v = 0; v < 2; ++v) {
        q[v] = *p;
        q[v].view = v ? WS_VIEW_RIGHT : WS_VIEW_LEFT;
        if (const int rc = check_params(err, &q[v], L, R); rc != WS_OK) return rc;
    }
    return WS_OK;
}

} // namespace

// Zeroed counters, the check kernel, the fill if asked for, and the counts on their way to the host -- all on s.
int enqueue_check(ws_context *ctx, LrMaps m, const ws_lr_params *lr, hipStream_t s)
{
    LrState &S = ctx->lr;
    int rc;
    const size_t slot_bytes = lr_slot_words() * sizeof(unsigned long long);
    if ((rc = S.counts.reserve(&ctx->err, slot_bytes)) != WS_OK) return rc;
    m.state[0] = m.state[1] = nullptr;
    if (lr->fill == WS_LR_FILL_BACKGROUND) {
        const size_t n0 = ((size_t)lr_state_pitch(m.w[0]) * m.h[0] + 255) & ~(size_t)255;
        if ((rc = ensure(&ctx->err, S.states, n0 + (size_t)lr_state_pitch(m.w[1]) * m.h[1])) != WS_OK) return rc;
        m.state[0] = static_cast<uint8_t *>(S.states.p);
        m.state[1] = m.state[0] + n0;
    }
    auto *slots = static_cast<unsigned long long *>(S.counts.dev.p), *counts = slots + lr_slot_words();
    WS_HIP(&ctx->err, hipMemsetAsync(slots, 0, slot_bytes, s));
    WS_HIP(&ctx->err, launch_lr_check(m, lr->max_diff, slots, counts, s));
    if (lr->fill == WS_LR_FILL_BACKGROUND) WS_HIP(&ctx->err, launch_lr_fill(m, s));
    return S.counts.fetch(&ctx->err, counts, s);
}

LrMaps lr_maps(const float *l, int lw, int lh, int lstride, const float *r, int rw, int rh, int rstride, float *ol, int olstride,
               float *orr, int orstride)
{
    LrMaps m{};
    m.in[0] = l; m.in[1] = r;
    m.out[0] = ol; m.out[1] = orr;
    m.w[0] = lw; m.h[0] = lh; m.w[1] = rw; m.h[1] = rh;
    m.in_pitch[0] = lstride; m.in_pitch[1] = rstride;
    m.out_pitch[0] = olstride; m.out_pitch[1] = orstride;
    return m;
}

// The scratch of ws_search_lr_*: both raw maps (dense), then (host form) both checked maps.  Offsets in floats.
int lr_maps_scratch(ws_context *ctx, size_t n_left, size_t n_right, int checked_too, float **base, size_t off[4])
{
    const auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
    off[0] = 0;
    off[1] = up(n_left);
    off[2] = off[1] + up(n_right);
    off[3] = off[2] + up(n_left);
    const size_t total = checked_too ? off[3] + n_right : off[1] + n_right;
    if (const int rc = ensure(&ctx->err, ctx->lr.raw, total * sizeof(float)); rc != WS_OK) return rc;
    *base = static_cast<float *>(ctx->lr.raw.p);
    return WS_OK;
}

namespace {

// Both views on the device images into the dense maps at base + off[0] (left) and base + off[1] (right), one after the
// other on s (they share the Searcher's scratch planes), then the check of the two into the maps m.out.
int search_and_check(ws_context *ctx, const ws_params q[2], const ws_image *L, const ws_image *R, float *base, const size_t off[4],
                     LrMaps m, const ws_lr_params *lr, hipStream_t s)
{
    int rc;
    if ((rc = search(ctx->searcher, &ctx->err, &q[0], L, R, base + off[0], L->width, nullptr, ctx->status_dev, s)) != WS_OK) return rc;
    if ((rc = search(ctx->searcher, &ctx->err, &q[1], L, R, base + off[1], R->width, nullptr, ctx->status_dev, s)) != WS_OK) return rc;
    return enqueue_check(ctx, m, lr, s);
}

} // namespace
} // namespace wsamd

using namespace wsamd;

extern "C" {

int ws_lr_check_device(ws_context *ctx, const float *left_dev, int lw, int lh, int lstride, const float *right_dev, int rw, int rh,
                       int rstride, const ws_lr_params *lr, float *out_left_dev, int out_lstride, float *out_right_dev,
                       int out_rstride, void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    int rc = check_lr(&ctx->err, lr);
    if (rc != WS_OK) return rc;
    if (!left_dev || !right_dev || !out_left_dev || !out_right_dev) return fail(&ctx->err, WS_ERR_ARG, "null map");
    if (lw < 1 || lh < 1 || rw < 1 || rh < 1 || lstride < lw || rstride < rw || out_lstride < lw || out_rstride < rw)
        return fail(&ctx->err, WS_ERR_ARG, "bad map size or stride");
    const Extent il = map_extent(left_dev, lw, lh, lstride), ir = map_extent(right_dev, rw, rh, rstride);
    const Extent ol = map_extent(out_left_dev, lw, lh, out_lstride), orr = map_extent(out_right_dev, rw, rh, out_rstride);
    if (ol.overlaps(il) || ol.overlaps(ir) || orr.overlaps(il) || orr.overlaps(ir) || ol.overlaps(orr))
        return fail(&ctx->err, WS_ERR_ARG, "an output map overlaps an input map or the other output");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    if ((rc = ctx->lr.lease.begin(&ctx->err, s)) != WS_OK) return rc;
    const LrMaps m = lr_maps(left_dev, lw, lh, lstride, right_dev, rw, rh, rstride, out_left_dev, out_lstride, out_right_dev, out_rstride);
    return ctx->lr.lease.end(&ctx->err, s, enqueue_check(ctx, m, lr, s));
}

int ws_search_lr_device(ws_context *ctx, const ws_params *p, const ws_image *left_dev, const ws_image *right_dev,
                        const ws_lr_params *lr, float *out_left_dev, int out_lstride, float *out_right_dev, int out_rstride,
                        void *stream)
{
    if (!ctx) return WS_ERR_ARG;
    ws_params q[2];
    int rc = view_params(&ctx->err, p, left_dev, right_dev, q);
    if (rc == WS_OK) rc = check_lr(&ctx->err, lr);
    if (rc != WS_OK) return rc;
    const int lw = left_dev->width, lh = left_dev->height, rw = right_dev->width, rh = right_dev->height;
    if (!out_left_dev || !out_right_dev) return fail(&ctx->err, WS_ERR_ARG, "null output");
    if (out_lstride < lw || out_rstride < rw) return fail(&ctx->err, WS_ERR_ARG, "output stride below the map's width");
    if (map_extent(out_left_dev, lw, lh, out_lstride).overlaps(map_extent(out_right_dev, rw, rh, out_rstride)))
        return fail(&ctx->err, WS_ERR_ARG, "the output maps overlap");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    float *base;
    size_t off[4];
    if ((rc = lr_maps_scratch(ctx, (size_t)lw * lh, (size_t)rw * rh, 0, &base, off)) != WS_OK) return rc;
    if ((rc = ctx->lr.lease.begin(&ctx->err, s)) != WS_OK) return rc;
    const LrMaps m = lr_maps(base + off[0], lw, lh, lw, base + off[1], rw, rh, rw, out_left_dev, out_lstride, out_right_dev, out_rstride);
    return ctx->lr.lease.end(&ctx->err, s, search_and_check(ctx, q, left_dev, right_dev, base, off, m, lr, s));
}

// As ws_search_host, twice, with the images uploaded once: both views into context scratch, the check beside them, and
// both checked maps down as float32, widened to the caller's type on the host.  One synchronisation at the end.
int ws_search_lr_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, const ws_lr_params *lr,
                      void *out_left, int out_lstride, void *out_right, int out_rstride, int out_dtype)
{
    if (!ctx) return WS_ERR_ARG;
    ws_params q[2];
    int owl, ohl, owr, ohr;
    int rc = view_params(&ctx->err, p, left, right, q);
    if (rc == WS_OK) rc = check_lr(&ctx->err, lr);
    if (rc == WS_OK) rc = check_out(&ctx->err, &q[0], left, right, out_left, out_lstride, out_dtype, &owl, &ohl);
    if (rc == WS_OK) rc = check_out(&ctx->err, &q[1], left, right, out_right, out_rstride, out_dtype, &owr, &ohr);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    hipStream_t s = call.s;
    float *base;
    size_t off[4];
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = lr_maps_scratch(ctx, (size_t)owl * ohl, (size_t)owr * ohr, 1, &base, off)) != WS_OK) return rc;
    const int esz = out_elem_size(out_dtype);
    span_set(sp[2], out_left, (size_t)out_lstride * esz, (size_t)owl * esz, (size_t)ohl, &ctx->h_out);
    span_set(sp[3], out_right, (size_t)out_rstride * esz, (size_t)owr * esz, (size_t)ohr, &ctx->h_aux[0]);
    spans_attach(sp, 4);
    rc = [&]() -> int {
        int r;
        if ((r = call.upload()) != WS_OK) return r;
        if ((r = ctx->lr.lease.begin(&ctx->err, s)) != WS_OK) return r;
        const LrMaps m = lr_maps(base + off[0], owl, ohl, owl, base + off[1], owr, ohr, owr, base + off[2], owl, base + off[3], owr);
        if ((r = ctx->lr.lease.end(&ctx->err, s, search_and_check(ctx, q, &call.dl, &call.dr, base, off, m, lr, s))) != WS_OK) return r;
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_lstride, base + off[2], (size_t)owl, (size_t)ohl, kWireF32, esz, s));
        WS_HIP(&ctx->err, span_download(sp[3], 0, (size_t)out_rstride, base + off[3], (size_t)owr, (size_t)ohr, kWireF32, esz, s));
        return WS_OK;
    }();
    return call.close(rc, 4, kWireF32, true, "left-right host call");
}

int ws_last_lr_counts(ws_context *ctx, unsigned long long counts[2])
{
    if (!ctx || !counts) return WS_ERR_ARG;
    return read_counts(ctx, ctx->lr.counts, ctx->lr.lease, "no left-right check has run on this context", counts);
}

} // extern "C"
