// ws_pair.cpp -- both views' maps and their cross-check from one cost volume (include/ws_stereo.h, extension): the base
// view's volumes and winner as ws_sgm.cpp runs them, the diagonal winner of ws_sgm.hip for the other view, and the
// left-right check of ws_lr.cpp on the two, on device memory or on the caller's host buffers (through ws_staging.h).
//
// Leases: the volumes and both winners run under the context's SGM lease; the raw maps in LrState::raw, the states and
// the check's counters under its left-right lease.  A call that needs both takes the SGM lease first and the
// left-right lease second, and ends them in the order it took them: no other call holds the two, and every call's
// begin() and end() happen inside that call on the host, so the order cannot deadlock -- it only fixes which stream
// waits for which.
#include "ws_context.h"
#include "ws_sgm.h"

#include <stdint.h>

namespace wsamd {
namespace {

int check_pair(std::string *err, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_lr_params *lr,
               const ws_image *L, const ws_image *R)
{
    if (const int rc = check_sgm(err, p, sgm, L, R, true); rc != WS_OK) return rc;
    if (uq)
        if (const int rc = check_ratio(err, uq); rc != WS_OK) return rc;
    return lr ? check_lr(err, lr) : WS_OK;
}

Extent map_extent(const void *p, int w, int h, int stride, int esz) { return Extent(p, (size_t)stride * esz, (size_t)w * esz, (size_t)h); }

// out_left is w1 x h1 and out_right w2 x h2 whichever view is the base; esz: the bytes of an element
int check_pair_out(std::string *err, const ws_image *L, const ws_image *R, const void *out_left, int out_lstride, const void *out_right,
                   int out_rstride, int esz)
{
    if (!out_left || !out_right) return fail(err, WS_ERR_ARG, "null output");
    if (out_lstride < L->width || out_rstride < R->width) return fail(err, WS_ERR_ARG, "output stride below the map's width");
    if (map_extent(out_left, L->width, L->height, out_lstride, esz).overlaps(map_extent(out_right, R->width, R->height, out_rstride, esz)))
        return fail(err, WS_ERR_ARG, "the output maps overlap");
    return WS_OK;
}

// The volumes of the base view, its winner into the base view's slot of raw[] and the diagonal winner into the other
// one, under the SGM lease; then, with lr, the check of raw[] into m.out under the left-right lease.  raw[0] is the left
// view's map (pitch rawp[0]), raw[1] the right view's.  lr_scratch: raw[] lies in LrState::raw, so the left-right lease
// is held whether or not the check runs.
int enqueue_pair(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_lr_params *lr,
                 const ws_image *L, const ws_image *R, float *const raw[2], const int rawp[2], LrMaps m, bool lr_scratch, hipStream_t s)
{
    const int base = p->view == WS_VIEW_RIGHT ? 1 : 0, other = 1 - base;
    const int wd = other ? R->width : L->width, hd = other ? R->height : L->height;
    ScratchLease &vol = ctx->sgm.lease, &chk = ctx->lr.lease;
    int rc;
    if ((rc = vol.begin(&ctx->err, s)) != WS_OK) return rc;
    if (lr_scratch && (rc = chk.begin(&ctx->err, s)) != WS_OK) return vol.end(&ctx->err, s, rc);
    rc = [&]() -> int {
        SgmArgs a;
        int r;
        if ((r = sgm_prepare(ctx, p, sgm, L, R, raw[base], rawp[base], s, &a)) != WS_OK) return r;
        if ((r = sgm_winner(ctx, a, sgm, uq, nullptr, 0, s)) != WS_OK) return r;
        WS_HIP(&ctx->err, launch_pair_wta(a, sgm ? sgm->paths : 0, raw[other], rawp[other], wd, hd, s));
        return WS_OK;
    }();
    rc = vol.end(&ctx->err, s, rc);
    if (!lr_scratch) return rc;
    return chk.end(&ctx->err, s, rc == WS_OK && lr ? enqueue_check(ctx, m, lr, s) : rc);
}

} // namespace
} // namespace wsamd

using namespace wsamd;

extern "C" {

int ws_validate_pair(const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_lr_params *lr,
                     const ws_image *left, const ws_image *right)
{
    return check_pair(nullptr, p, sgm, uq, lr, left, right);
}

int ws_search_pair_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                          const ws_lr_params *lr, const ws_image *left_dev, const ws_image *right_dev, float *out_left_dev,
                          int out_lstride, float *out_right_dev, int out_rstride, void *stream)
{
    // (the refusals come before the context is looked at: they are the rules', and need no device)
    std::string *err = ctx ? &ctx->err : nullptr;
    int rc = check_pair(err, p, sgm, uq, lr, left_dev, right_dev);
    if (rc == WS_OK) rc = check_pair_out(err, left_dev, right_dev, out_left_dev, out_lstride, out_right_dev, out_rstride, 4);
    if (rc != WS_OK) return rc;
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    const int lw = left_dev->width, lh = left_dev->height, rw = right_dev->width, rh = right_dev->height;
    float *raw[2] = {out_left_dev, out_right_dev}; // without lr the kernels write the caller's maps
    int rawp[2] = {out_lstride, out_rstride};
    LrMaps m{};
    if (lr) {
        float *base;
        size_t off[4];
        if ((rc = lr_maps_scratch(ctx, (size_t)lw * lh, (size_t)rw * rh, 0, &base, off)) != WS_OK) return rc;
        raw[0] = base + off[0]; raw[1] = base + off[1];
        rawp[0] = lw; rawp[1] = rw;
        m = lr_maps(raw[0], lw, lh, lw, raw[1], rw, rh, rw, out_left_dev, out_lstride, out_right_dev, out_rstride);
    }
    return enqueue_pair(ctx, p, sgm, uq, lr, left_dev, right_dev, raw, rawp, m, lr != nullptr, s);
}

// As ws_search_lr_host: the images up once, both raw maps into LrState::raw (with lr: the checked maps beside them), and
// the two maps down as float32, widened to the caller's type on the host.  One synchronisation at the end.
int ws_search_pair_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                        const ws_lr_params *lr, const ws_image *left, const ws_image *right, void *out_left, int out_lstride,
                        void *out_right, int out_rstride, int out_dtype)
{
    std::string *err = ctx ? &ctx->err : nullptr;
    int rc = check_pair(err, p, sgm, uq, lr, left, right);
    if (rc != WS_OK) return rc;
    if (out_dtype != WS_OUT_F32 && out_dtype != WS_OUT_F64) return fail(err, WS_ERR_ARG, "bad output");
    const int esz = out_elem_size(out_dtype);
    if ((rc = check_pair_out(err, left, right, out_left, out_lstride, out_right, out_rstride, esz)) != WS_OK) return rc;
    if (!ctx) return fail(nullptr, WS_ERR_ARG, "null context");
    WS_HIP(&ctx->err, hipSetDevice(ctx->device));
    const int lw = left->width, lh = left->height, rw = right->width, rh = right->height;
    PairHostCall call(ctx, left, right);
    HostSpan *sp = call.sp;
    hipStream_t s = call.s;
    float *base;
    size_t off[4];
    if ((rc = call.open()) != WS_OK) return rc;
    if ((rc = lr_maps_scratch(ctx, (size_t)lw * lh, (size_t)rw * rh, lr ? 1 : 0, &base, off)) != WS_OK) return rc;
    span_set(sp[2], out_left, (size_t)out_lstride * esz, (size_t)lw * esz, (size_t)lh, &ctx->h_out);
    span_set(sp[3], out_right, (size_t)out_rstride * esz, (size_t)rw * esz, (size_t)rh, &ctx->h_aux[0]);
    spans_attach(sp, 4);
    rc = [&]() -> int {
        int r;
        if ((r = call.upload()) != WS_OK) return r;
        float *raw[2] = {base + off[0], base + off[1]};
        const int rawp[2] = {lw, rw};
        const float *dl = raw[0], *dr = raw[1]; // what goes down: the raw maps, or with lr the checked ones
        LrMaps m{};
        if (lr) {
            m = lr_maps(raw[0], lw, lh, lw, raw[1], rw, rh, rw, base + off[2], lw, base + off[3], rw);
            dl = base + off[2];
            dr = base + off[3];
        }
        if ((r = enqueue_pair(ctx, p, sgm, uq, lr, &call.dl, &call.dr, raw, rawp, m, true, s)) != WS_OK) return r;
        WS_HIP(&ctx->err, span_download(sp[2], 0, (size_t)out_lstride, dl, (size_t)lw, (size_t)lh, kWireF32, esz, s));
        WS_HIP(&ctx->err, span_download(sp[3], 0, (size_t)out_rstride, dr, (size_t)rw, (size_t)rh, kWireF32, esz, s));
        return WS_OK;
    }();
    return call.close(rc, 4, kWireF32, false, "pair host call");
}

} // extern "C"
