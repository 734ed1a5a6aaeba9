// ws_capi_internal.h -- what the sources of the C-ABI share that is not part of it: error reporting, device scratch
// memory and the lease that orders its users across streams, the map's size and the overlap test, and the entry points
// of ws_capi.cpp that other sources call.
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#pragma GCC visibility push(hidden) // (internal to the library: nothing here is exported)
namespace wsamd {

// Record an error message and return `code`: into *err (a context's error string), or with err == nullptr into this
// thread's message that ws_last_error(NULL) returns.
int fail(std::string *err, int code, const char *fmt, ...);

#define WS_HIP(err, call)                                                                                            \
    do {                                                                                                             \
        if (const hipError_t e_ = (call); e_ != hipSuccess)                                                          \
            return wsamd::fail(err, WS_ERR_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// device memory of a context (ensure), freed with its owner: ws_destroy makes the context's device current and its
// streams idle before it deletes the context
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// at least `bytes` in b (grown with headroom; the old contents are not kept)
inline int ensure(std::string *err, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return WS_OK;
    if (b.p) WS_HIP(err, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    WS_HIP(err, hipMalloc(&b.p, want));
    b.cap = want;
    return WS_OK;
}

// A lease on scratch that every call of one kind shares across streams: the Searcher's planes, the
// left-right check's, the speckle filter's and SGM's scratch hold one each.  begin() before the first operation that
// touches the scratch, end() behind the last one, on every path out of the call.
struct ScratchLease {
    hipEvent_t ev = nullptr; // end of the last call (created by the first)
    hipStream_t stream = nullptr;
    bool busy = false; // ev is recorded on `stream`
    ScratchLease() = default;
    ScratchLease(const ScratchLease &) = delete;
    ScratchLease &operator=(const ScratchLease &) = delete;
    ~ScratchLease() { if (ev) (void)hipEventDestroy(ev); }
    // a call on another stream than the previous one first waits for it (on the device)
    int begin(std::string *err, hipStream_t s)
    {
        if (!ev) WS_HIP(err, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (busy && s != stream) WS_HIP(err, hipStreamWaitEvent(s, ev, 0));
        return WS_OK;
    }
    // rc: what the call's body returned, and what end() returns unless the body succeeded and the record failed
    int end(std::string *err, hipStream_t s, int rc)
    {
        busy = false;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cap);
        if (cap != hipStreamCaptureStatusNone) return rc; // (an event recorded inside a capture cannot be waited for outside it)
        if (const hipError_t e = hipEventRecord(ev, s); e != hipSuccess)
            return rc != WS_OK ? rc : fail(err, WS_ERR_HIP, "hipEventRecord (scratch lease): %s", hipGetErrorString(e));
        busy = true;
        stream = s;
        return rc;
    }
};

// The map of the search p on L, R: the left view's is the left image's size, every other view's the right image's.
inline void map_dims(const ws_params *p, const ws_image *L, const ws_image *R, int *w, int *h)
{
    *w = p->view == WS_VIEW_LEFT ? L->width : R->width;
    *h = p->view == WS_VIEW_LEFT ? L->height : R->height;
}

inline int out_elem_size(int out_dtype) { return out_dtype == WS_OUT_F32 ? 4 : 8; } // bytes of a WS_OUT_F32 / WS_OUT_F64 element

// the bytes [lo, hi) a plane of `rows` rows of `row_bytes`, `pitch` bytes apart, occupies
struct Extent {
    uintptr_t lo, hi;
    Extent(const void *p, size_t pitch, size_t row_bytes, size_t rows)
        : lo(reinterpret_cast<uintptr_t>(p)), hi(lo + pitch * (rows - 1) + row_bytes) {}
    bool overlaps(const Extent &o) const { return lo < o.hi && o.lo < hi; }
};

// ws_enqueue_host for the map rows [map_row0, map_row0 + map_rows) only (map_rows < 0: the whole map); `out` points at
// where map row map_row0 lands.  Ends with ws_wait like ws_enqueue_host.
int enqueue_host_rows(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, void *out,
                      int out_stride, int out_dtype, int map_row0, int map_rows);

} // namespace wsamd
#pragma GCC visibility pop
