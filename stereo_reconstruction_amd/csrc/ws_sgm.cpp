// ws_sgm.cpp -- semi-global matching of include/ws_stereo.h (extension): argument checks, the storage widths from the
// host's bound, the context's scratch for it (SgmState), and the launches of ws_sgm.hip on device memory or on the
// caller's host buffers (through ws_staging.h).  Also the uniqueness ratio and confidence calls (ws_search_unique_*):
// the same volumes with another winner kernel, on S or -- without a ws_sgm_params -- on the window costs themselves.
#include "ws_context.h"
#include "ws_ct.h"
#include "ws_sgm.h"

#include <stdint.h>

#include <algorithm>

namespace wsamd {

int check_sgm(std::string *err, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R, bool sgm_optional)
{
    if (const int rc = check_params(err, p, L, R); rc != WS_OK) return rc;
    if (p->view == WS_VIEW_LINEAR) return fail(err, WS_ERR_UNSUPPORTED, "SGM on LinearSearch");
    if (p->smooth_factor != 1.0) return fail(err, WS_ERR_UNSUPPORTED, "SGM together with smoothFactor != 1");
    if (p->view == WS_VIEW_RIGHT && p->var_block) return fail(err, WS_ERR_UNSUPPORTED, "SGM together with varBlock");
    if (!sgm && !sgm_optional) return fail(err, WS_ERR_ARG, "null ws_sgm_params");
    if (sgm) {
        if (sgm->paths != 4 && sgm->paths != 8) return fail(err, WS_ERR_ARG, "paths %d: must be 4 or 8", sgm->paths);
        if (sgm->p1 < 0) return fail(err, WS_ERR_ARG, "p1 %d: must be >= 0", sgm->p1);
        if (sgm->p2 < sgm->p1) return fail(err, WS_ERR_ARG, "p2 %d: must be >= p1 (%d)", sgm->p2, sgm->p1);
    }
    int d0, nd;
    disparity_range(p, L, &d0, &nd);
    if (nd > kSgmMaxNd) return fail(err, WS_ERR_UNSUPPORTED, "SGM over %d disparities: at most %d", nd, kSgmMaxNd);
    int w, h;
    map_dims(p, L, R, &w, &h);
    if ((long long)w * h >= (1LL << 31)) return fail(err, WS_ERR_UNSUPPORTED, "SGM on a map of 2^31 pixels or more");
    return WS_OK;
}

int check_ratio(std::string *err, const ws_unique_params *uq)
{
    if (uq->ratio < 0 || uq->ratio > 100) return fail(err, WS_ERR_ARG, "ratio %d: must be 0 .. 100", uq->ratio);
    return WS_OK;
}

namespace {

int check_unique(std::string *err, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_image *L,
                 const ws_image *R)
{
    if (const int rc = check_sgm(err, p, sgm, L, R, true); rc != WS_OK) return rc;
    if (!uq) return fail(err, WS_ERR_ARG, "null ws_unique_params");
    return check_ratio(err, uq);
}

// The scratch of one call: the candidate intervals, the cost plane and the sums (none without sgm: the uniqueness calls'
// block route), each 256-byte aligned.  Storage
// widths from the bound: C <= Cmax = 3 (255 or 255^2) bs^2 < 2^30 (a census cost: 24 or 62 bs^2); Lr <= C + P2 < 2^32; S <= paths (Cmax + P2).
struct Layout {
    int d0 = 0, nd = 0, w = 0, h = 0, cost16 = 0, sum64 = 0;
    size_t off_cost = 0, off_sum = 0, off_tl = 0, off_tr = 0, bytes = 0; // (off_tl, off_tr: a census cost's descriptor planes)
};

Layout layout(const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R)
{
    Layout y;
    disparity_range(p, L, &y.d0, &y.nd);
    map_dims(p, L, R, &y.w, &y.h);
    const uint64_t cmax = sgm_cost_max(p->cost, p->block_size);
    y.cost16 = cmax <= 0xffffu;
    y.sum64 = sgm && (uint64_t)sgm->paths * (cmax + (uint64_t)sgm->p2) > 0xffffffffull;
    const auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t px = (size_t)y.w * y.h, vol = px * (size_t)y.nd;
    y.off_cost = up(px * 4);
    y.off_sum = y.off_cost + up(vol * (y.cost16 ? 2 : 4));
    y.bytes = y.off_sum + (sgm ? up(vol * (y.sum64 ? 8 : 4)) : 0);
    if (is_census(p->cost)) {
        const size_t esz = census_plane_elem(p->cost);
        y.off_tl = y.bytes;
        y.off_tr = y.off_tl + up((size_t)L->width * L->height * esz);
        y.bytes = y.off_tr + up((size_t)R->width * R->height * esz);
    }
    return y;
}

// Grown to exactly what the call needs (the volumes are large: no headroom).  A failed allocation leaves the context
// without SGM scratch and usable.
int sgm_ensure(ws_context *ctx, size_t bytes)
{
    DevBuf &b = ctx->sgm.scratch;
    if (bytes <= b.cap) return WS_OK;
    if (b.p) WS_HIP(&ctx->err, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(&ctx->err, WS_ERR_NOMEM, "SGM scratch of %zu bytes could not be allocated", bytes);
    }
    b.cap = bytes;
    return WS_OK;
}

} // namespace

int sgm_prepare(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R, float *out,
                int out_stride, hipStream_t s, SgmArgs *args)
{
    const Layout y = layout(p, sgm, L, R);
    // (a grown buffer is freed and allocated again: hipFree waits for the work still using the old one)
    if (const int rc = sgm_ensure(ctx, y.bytes); rc != WS_OK) return rc;
    SgmArgs a{};
    a.L = L->data; a.R = R->data;
    a.w1 = L->width; a.h1 = L->height; a.s1 = L->stride;
    a.w2 = R->width; a.h2 = R->height; a.s2 = R->stride;
    a.right = p->view == WS_VIEW_RIGHT;
    a.ssd = p->cost == WS_COST_SSD;
    a.half = (p->block_size - 1) / 2;
    a.d0 = y.d0; a.nd = y.nd;
    a.w = y.w; a.h = y.h;
    if (sgm) { a.p1 = (uint32_t)sgm->p1; a.p2 = (uint32_t)sgm->p2; }
    auto *base = static_cast<uint8_t *>(ctx->sgm.scratch.p);
    a.kr = reinterpret_cast<uint32_t *>(base);
    a.cost = base + y.off_cost;
    a.sum = sgm ? base + y.off_sum : nullptr;
    a.cost16 = y.cost16; a.sum64 = y.sum64;
    if (is_census(p->cost)) {
        a.TL = base + y.off_tl;
        a.TR = base + y.off_tr;
        a.census_wide = p->cost == WS_COST_CENSUS_9X7;
        WS_HIP(&ctx->err, launch_census_transform(L->data, L->width, L->height, L->stride, p->cost, base + y.off_tl, L->width, false, s));
        WS_HIP(&ctx->err, launch_census_transform(R->data, R->width, R->height, R->stride, p->cost, base + y.off_tr, R->width, false, s));
    }
    a.subpixel = p->subpixel != 0;
    a.out = out;
    a.out_pitch = out_stride;
    *args = a;
    return WS_OK;
}

int sgm_winner(ws_context *ctx, const SgmArgs &a, const ws_sgm_params *sgm, const ws_unique_params *uq, float *conf, int conf_stride,
               hipStream_t s)
{
    if (uq) {
        SgmState &S = ctx->sgm;
        if (const int rc = S.counts.reserve(&ctx->err, 0); rc != WS_OK) return rc;
        UniqueArgs u{};
        u.ratio = uq->ratio;
        u.conf = conf;
        u.conf_pitch = conf_stride;
        u.counts = static_cast<unsigned long long *>(S.counts.dev.p);
        u.num_cus = ctx->num_cus;
        WS_HIP(&ctx->err, hipMemsetAsync(u.counts, 0, CountPair::kBytes, s));
        WS_HIP(&ctx->err, launch_unique(a, u, sgm ? sgm->paths : 0, s));
        return S.counts.fetch(&ctx->err, u.counts, s);
    }
    WS_HIP(&ctx->err, launch_sgm(a, sgm ? sgm->paths : 0, s));
    return WS_OK;
}

namespace {

// Scratch, then the kernels on s into out (out_stride floats per row).  uq: the uniqueness winner instead (sgm may then
// be null), with the confidence plane conf (or null) and the counts on their way to the host.
int sgm_on(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R, float *out,
           int out_stride, hipStream_t s, const ws_unique_params *uq, float *conf, int conf_stride)
{
    SgmArgs a;
    if (const int rc = sgm_prepare(ctx, p, sgm, L, R, out, out_stride, s, &a); rc != WS_OK) return rc;
    return sgm_winner(ctx, a, sgm, uq, conf, conf_stride, s);
}

// ... under the lease of the context's SGM scratch (before the scratch is grown: the old one may still be in use)
int enqueue_sgm(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *L, const ws_image *R, float *out,
                int out_stride, hipStream_t s, const ws_unique_params *uq = nullptr, float *conf = nullptr, int conf_stride = 0)
{
    ScratchLease &lease = ctx->sgm.lease;
    if (const int rc = lease.begin(&ctx->err, s); rc != WS_OK) return rc;
    return lease.end(&ctx->err, s, sgm_on(ctx, p, sgm, L, R, out, out_stride, s, uq, conf, conf_stride));
}

} // namespace
} // namespace wsamd

using namespace wsamd;

extern "C" {

int ws_validate_sgm(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right)
{
    return check_sgm(nullptr, p, sgm, left, right);
}

int ws_sgm_scratch_bytes(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right,
                         unsigned long long *bytes)
{
    if (!bytes) return fail(nullptr, WS_ERR_ARG, "null bytes");
    if (const int rc = check_sgm(nullptr, p, sgm, left, right); rc != WS_OK) return rc;
    *bytes = layout(p, sgm, left, right).bytes;
    return WS_OK;
}

int ws_search_sgm_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *left_dev,
                         const ws_image *right_dev, float *out_dev, int out_stride, void *stream)
{
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    int rc = check_sgm(&ctx->err, p, sgm, left_dev, right_dev);
    if (rc != WS_OK) return rc;
    int ow, oh;
    map_dims(p, left_dev, right_dev, &ow, &oh);
    if (!out_dev) return fail(&ctx->err, WS_ERR_ARG, "null output");
    if (out_stride < ow) return fail(&ctx->err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return enqueue_sgm(ctx, p, sgm, left_dev, right_dev, out_dev, out_stride, s);
}

// As ws_search_host: both images up (through the shared staging path), the search on the context's stream into a dense
// float32 map, and the map down, widened to the caller's type on the host.  One synchronisation at the end.
int ws_search_sgm_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *left,
                       const ws_image *right, void *out, int out_stride, int out_dtype)
{
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    int ow, oh;
    int rc = check_sgm(&ctx->err, p, sgm, left, right);
    if (rc == WS_OK) rc = check_out(&ctx->err, p, left, right, out, out_stride, out_dtype, &ow, &oh);
    if (rc != WS_OK) return rc;
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    hipStream_t s = call.s;
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, (size_t)ow * oh * sizeof(float))) != WS_OK) return rc;
    const int esz = out_elem_size(out_dtype);
    span_set(sp[2], out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)oh, &ctx->h_out);
    spans_attach(sp, 3);
    rc = [&]() -> int {
        int r;
        if ((r = call.upload()) != WS_OK) return r;
        float *map = static_cast<float *>(ctx->d_out.p);
        if ((r = enqueue_sgm(ctx, p, sgm, &call.dl, &call.dr, map, ow, s)) != WS_OK) return r;
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_stride, map, (size_t)ow, (size_t)oh, kWireF32, esz, s));
        return WS_OK;
    }();
    return call.close(rc, 3, kWireF32, false, "SGM host call");
}

int ws_validate_unique(const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_image *left,
                       const ws_image *right)
{
    return check_unique(nullptr, p, sgm, uq, left, right);
}

int ws_unique_scratch_bytes(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right,
                            unsigned long long *bytes)
{
    if (!bytes) return fail(nullptr, WS_ERR_ARG, "null bytes");
    if (const int rc = check_sgm(nullptr, p, sgm, left, right, true); rc != WS_OK) return rc;
    *bytes = layout(p, sgm, left, right).bytes;
    return WS_OK;
}

int ws_search_unique_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                            const ws_image *left_dev, const ws_image *right_dev, float *out_dev, int out_stride, float *conf_dev,
                            int conf_stride, void *stream)
{
    // (the refusals come before the context is looked at: they are the rules', and need no device)
    std::string *err = ctx ? &ctx->err : nullptr;
    int rc = check_unique(err, p, sgm, uq, left_dev, right_dev);
    if (rc != WS_OK) return rc;
    int ow, oh;
    map_dims(p, left_dev, right_dev, &ow, &oh);
    if (!out_dev) return fail(err, WS_ERR_ARG, "null output");
    if (out_stride < ow) return fail(err, WS_ERR_ARG, "out_stride %d < width %d", out_stride, ow);
    if (conf_dev) {
        if (conf_stride < ow) return fail(err, WS_ERR_ARG, "conf_stride %d < width %d", conf_stride, ow);
        const Extent map(out_dev, (size_t)out_stride * 4, (size_t)ow * 4, (size_t)oh), cf(conf_dev, (size_t)conf_stride * 4, (size_t)ow * 4, (size_t)oh);
        if (map.overlaps(cf))
            return fail(err, WS_ERR_ARG, "the confidence plane overlaps the map");
    }
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    return enqueue_sgm(ctx, p, sgm, left_dev, right_dev, out_dev, out_stride, s, uq, conf_dev, conf_stride);
}

// As ws_search_sgm_host; the confidence plane, when asked for, beside the map in d_out and down as float32.
int ws_search_unique_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                          const ws_image *left, const ws_image *right, void *out, int out_stride, int out_dtype, float *conf,
                          int conf_stride)
{
    std::string *err = ctx ? &ctx->err : nullptr;
    int ow, oh;
    int rc = check_unique(err, p, sgm, uq, left, right);
    if (rc == WS_OK) rc = check_out(err, p, left, right, out, out_stride, out_dtype, &ow, &oh);
    if (rc != WS_OK) return rc;
    const int esz = out_elem_size(out_dtype);
    if (conf) {
        if (conf_stride < ow) return fail(err, WS_ERR_ARG, "conf_stride %d < width %d", conf_stride, ow);
        const Extent map(out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)oh), cf(conf, (size_t)conf_stride * 4, (size_t)ow * 4, (size_t)oh);
        if (map.overlaps(cf))
            return fail(err, WS_ERR_ARG, "the confidence plane overlaps the map");
    }
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    const size_t px = (size_t)ow * oh;
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    hipStream_t s = call.s;
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = ensure(&ctx->err, ctx->d_out, (conf ? 2 : 1) * px * sizeof(float))) != WS_OK) return rc;
    span_set(sp[2], out, (size_t)out_stride * esz, (size_t)ow * esz, (size_t)oh, &ctx->h_out);
    if (conf) span_set(sp[3], conf, (size_t)conf_stride * 4, (size_t)ow * 4, (size_t)oh, &ctx->h_aux[0]);
    spans_attach(sp, 4);
    rc = [&]() -> int {
        int r;
        if ((r = call.upload()) != WS_OK) return r;
        float *map = static_cast<float *>(ctx->d_out.p), *cmap = conf ? map + px : nullptr;
        if ((r = enqueue_sgm(ctx, p, sgm, &call.dl, &call.dr, map, ow, s, uq, cmap, ow)) != WS_OK) return r;
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_stride, map, (size_t)ow, (size_t)oh, kWireF32, esz, s));
        if (conf) WS_HIP(&ctx->err, span_download(sp[3], 0, (size_t)conf_stride, cmap, (size_t)ow, (size_t)oh, kWireF32, 4, s));
        return WS_OK;
    }();
    return call.close(rc, 4, kWireF32, false, "uniqueness host call");
}

int ws_last_unique_counts(ws_context *ctx, unsigned long long counts[2])
{
    if (!ctx || !counts) return WS_ERR_ARG;
    return read_counts(ctx, ctx->sgm.counts, ctx->sgm.lease, "no uniqueness call has run on this context", counts);
}

} // extern "C"
