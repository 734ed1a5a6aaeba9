// ws_capi_internal.h -- what the sources of the C-ABI share that is not part of it: error reporting, device scratch
// memory, and the entry points of ws_capi.cpp that other sources call.
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>
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

// ws_enqueue_host for the map rows [map_row0, map_row0 + map_rows) only (map_rows < 0: the whole map); `out` points at
// where map row map_row0 lands.  Ends with ws_wait like ws_enqueue_host.
int enqueue_host_rows(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, void *out,
                      int out_stride, int out_dtype, int map_row0, int map_rows);

} // namespace wsamd
#pragma GCC visibility pop
