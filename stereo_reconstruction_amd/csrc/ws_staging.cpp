// ws_staging.cpp -- the copies between the caller's host buffers and the device (ws_staging.h).
#include "ws_staging.h"
#include "ws_copy_pool.h"

#include <string.h>

namespace wsamd {

namespace {

// rows of `width_bytes` between buffers with row pitches: one linear copy when both sides are dense
// (the runtime's 2-D path is slow, very slow for row lengths that are not a multiple of 4 bytes)
hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t rows,
                     hipMemcpyKind kind, hipStream_t s)
{
    if (dpitch == width_bytes && spitch == width_bytes) return hipMemcpyAsync(dst, src, width_bytes * rows, kind, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, rows, kind, s);
}

bool runtime_knows(uintptr_t q)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, reinterpret_cast<const void *>(q)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type != hipMemoryTypeUnregistered;
}

size_t wire_bytes(int wire, int esz) { return wire == kWireI16 ? 2 : wire == kWireF32 ? 4 : (size_t)esz; }

hipError_t stage_for(HostSpan &sp)
{
    if (!sp.stage) return hipErrorInvalidValue;
    return host_ensure(*sp.stage, sp.n);
}

// A narrow cut-out of a much wider image goes through a pinned buffer of the library's own: the rows are gathered
// on the host and cross as one dense linear copy.  (The runtime's 2-D copy from pageable memory takes a per-row
// path, ~15 us a row; and no copy of this library reads or writes pageable memory through the runtime any more,
// see DESIGN.md 5.)
hipError_t gather_rows(HostBuf &b, const ws_image *im)
{
    const size_t rb = (size_t)im->width * 3;
    hipError_t e = host_ensure(b, rb * im->height);
    if (e != hipSuccess) return e;
    for (int y = 0; y < im->height; ++y) memcpy(b.p + (size_t)y * rb, im->data + (size_t)y * im->stride, rb);
    return hipSuccess;
}

} // namespace

bool linear_span(const ws_image *im)
{
    const size_t dense = (size_t)im->width * 3 * im->height;
    const size_t span = (size_t)im->stride * (im->height - 1) + (size_t)im->width * 3;
    return span <= 2 * dense || span <= ((size_t)32 << 20);
}

hipError_t host_ensure(HostBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return hipSuccess;
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&b.p), want, hipHostMallocDefault);
    if (e == hipSuccess) b.cap = want;
    return e;
}

void spans_attach(HostSpan *sp, int count)
{
    for (int i = 0; i < count; ++i) {
        if (!sp[i].p || !sp[i].n) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(sp[i].p);
        const bool k0 = runtime_knows(a), k1 = runtime_knows(a + sp[i].n - 1);
        // (staged: pageable memory -- this library registers no caller memory -- or a range the runtime knows in part)
        sp[i].how = k0 && k1 ? HostSpan::kCallerPinned : HostSpan::kStaged;
    }
}

hipError_t span_upload(HostSpan &sp, size_t off, void *dev, size_t bytes, hipStream_t s)
{
    if (off + bytes > sp.n) return hipErrorInvalidValue;
    if (sp.how == HostSpan::kCallerPinned) {
        const hipError_t e = hipMemcpyAsync(dev, sp.p + off, bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) return e;
        (void)hipGetLastError(); // caller-pinned memory the runtime will not copy from as one range: through the stage
        sp.how = HostSpan::kStaged;
    }
    if (sp.how != HostSpan::kStaged) return hipErrorInvalidValue;
    // just the bytes asked for, at their own offset in the stage (which is as long as the buffer): a call that uploads
    // its images band by band copies the next band into the stage while the last one is on the bus
    const hipError_t e = stage_for(sp);
    if (e != hipSuccess) return e;
    CopyPool::get().copy(sp.stage->p + off, sp.p + off, bytes);
    return hipMemcpyAsync(dev, sp.stage->p + off, bytes, hipMemcpyHostToDevice, s);
}

hipError_t span_upload_rows(HostSpan &sp, size_t off, size_t pitch, void *dev, size_t row_bytes, size_t rows, hipStream_t s)
{
    if (!rows || !row_bytes) return hipSuccess;
    if (off + pitch * (rows - 1) + row_bytes > sp.n) return hipErrorInvalidValue;
    if (pitch == row_bytes) return span_upload(sp, off, dev, row_bytes * rows, s);
    if (sp.how == HostSpan::kCallerPinned) {
        const hipError_t e = hipMemcpy2DAsync(dev, row_bytes, sp.p + off, pitch, row_bytes, rows, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) return e;
        (void)hipGetLastError(); // (as in span_upload)
        sp.how = HostSpan::kStaged;
    }
    if (sp.how != HostSpan::kStaged) return hipErrorInvalidValue;
    const hipError_t e = stage_for(sp);
    if (e != hipSuccess) return e;
    for (size_t r = 0; r < rows; ++r) memcpy(sp.stage->p + r * row_bytes, sp.p + off + r * pitch, row_bytes); // dense in the stage
    return hipMemcpyAsync(dev, sp.stage->p, row_bytes * rows, hipMemcpyHostToDevice, s);
}

hipError_t span_download(HostSpan &sp, size_t off, size_t pitch, const void *dev, size_t row_elems, size_t rows, int wire, int esz, hipStream_t s)
{
    if (!rows || !row_elems) return hipSuccess;
    if ((off + pitch * (rows - 1) + row_elems) * (size_t)esz > sp.n) return hipErrorInvalidValue;
    const size_t wb = wire_bytes(wire, esz);
    const bool same = wb == (size_t)esz; // (float32 on the wire for a float32 map)
    if (sp.how == HostSpan::kCallerPinned && same) {
        const hipError_t e = copy_rows(sp.p + off * esz, pitch * esz, dev, row_elems * esz, row_elems * esz, rows, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) return e;
        (void)hipGetLastError(); // caller-pinned memory the runtime will not copy to as one range: through the stage
        sp.how = HostSpan::kStaged;
    }
    if (sp.how != HostSpan::kStaged && sp.how != HostSpan::kCallerPinned) return hipErrorInvalidValue;
    const hipError_t e = stage_for(sp);
    if (e != hipSuccess) return e;
    // dense in the stage, at the wire-format offset of its first element (the stage is as long as the buffer)
    sp.down.push_back({off * wb, off * (size_t)esz, row_elems, rows, pitch * (size_t)esz, same ? (int)kWireSame : wire, esz});
    return hipMemcpyAsync(sp.stage->p + off * wb, dev, row_elems * wb * rows, hipMemcpyDeviceToHost, s);
}

hipError_t span_download_bytes(HostSpan &sp, size_t off, size_t pitch, const void *dev, size_t row_bytes, size_t rows, hipStream_t s)
{
    return span_download(sp, off, pitch, dev, row_bytes, rows, kWireSame, 1, s);
}

void span_scatter_seg(HostSpan &sp, HostSpan::Seg &g)
{
    if (!g.rows) return; // handed over already
    const CopyKind kind = g.wire == kWireI16 ? (g.esz == 8 ? kCopyI16F64 : kCopyI16F32) : g.wire == kWireF32 && g.esz == 8 ? kCopyF32F64 : kCopyBytes;
    const size_t unit = kind == kCopyBytes ? (size_t)g.esz : 1; // kCopyBytes counts bytes, the widening kinds elements
    const size_t wb = wire_bytes(g.wire, g.esz);
    if (g.host_pitch == g.row_elems * (size_t)g.esz || g.rows == 1) { // dense: one copy
        CopyPool::get().copy(sp.p + g.host_off, sp.stage->p + g.stage_off, g.row_elems * g.rows * unit, kind);
    } else {
        for (size_t r = 0; r < g.rows; ++r)
            copy_piece(sp.p + g.host_off + r * g.host_pitch, sp.stage->p + g.stage_off + r * g.row_elems * wb, 0, g.row_elems * unit, kind);
    }
    g.rows = 0;
}

void span_scatter(HostSpan &sp)
{
    for (HostSpan::Seg &g : sp.down) span_scatter_seg(sp, g);
    sp.down.clear();
}

void spans_finish(HostSpan *sp, int count)
{
    for (int i = 0; i < count; ++i) {
        span_scatter(sp[i]);
        sp[i].how = HostSpan::kUnused;
    }
}

size_t image_span(HostSpan &sp, const ws_image *im, HostBuf *stage)
{
    sp.stage = stage;
    const size_t rb = (size_t)im->width * 3;
    if (!linear_span(im)) return rb * im->height;
    span_set(sp, im->data, im->stride, rb, im->height, stage);
    return sp.n;
}

hipError_t upload_image(HostSpan &sp, const ws_image *im, uint8_t *dev, hipStream_t s, ws_image *dev_im)
{
    *dev_im = ws_image{dev, im->width, im->height, im->stride};
    if (sp.n) return span_upload(sp, 0, dev, sp.n, s);
    // (gathered into the stage: a synchronous call ends with a synchronisation, a job slot waits for its previous
    // upload, so the stage is free again when the next image is gathered)
    dev_im->stride = im->width * 3;
    const hipError_t e = gather_rows(*sp.stage, im);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(dev, sp.stage->p, (size_t)dev_im->stride * im->height, hipMemcpyHostToDevice, s);
}

} // namespace wsamd
