// ws_staging.h -- how the bytes of a caller's host buffers cross to and from the device: pinned stages of the library's
// own, caller-pinned memory used as it is, gathered rows of cut-out images, and the wire format of a disparity map.
// Knows HIP and ws_image, not ws_context: the context owns the stages and hands them to the spans of a call.
#pragma once

#include "../../include/ws_stereo.h"

#include <hip/hip_runtime.h>

#include <vector>

#pragma GCC visibility push(hidden) // (internal to the library: nothing here is exported)
namespace wsamd {

// ---- caller host buffers ----------------------------------------------------------------------------------------
// This library registers NO caller memory (no hipHostRegister / hipHostUnregister anywhere in it).  Round 2 registered
// the caller's buffers for the duration of a call; round 3 found what that costs inside somebody else's process -- the
// runtime abort()s on an unregister of a pointer that lies inside another live registration (rocclr device.cpp:373,
// tools/ubench/hostreg_probe.hip, profiles/r03/hostreg_probe.txt), and two full test runs ended in a GPU memory fault on
// a host heap page whose cause was never proven -- and made it opt-in; round 4 removed it: the 16-bit
// wire format below wins back more than the registration saved.  How bytes cross now:
//   * pageable memory (a cv::Mat, a numpy array) crosses through pinned staging memory of the library's own
//     (hipHostMalloc): one host copy each way, on a small pool of threads, band by band beside the transfers;
//   * memory the runtime already knows at both ends -- the caller's own hipHostMalloc / hipHostRegister, a framework's
//     pinned allocator -- is used as it is, never registered or released here;
//   * a range the runtime knows only in part goes through the stage (a direct copy across its edge would be refused).
// Never through the runtime's pageable copy path: it blocks the calling thread for the whole transfer
// (profiles/r02/pcie_probe.txt).
//
// WIRE FORMAT of a disparity map: every value a search stores is an integer in [-w, max(maxDisparity, w)]
// (BlockSearch.cpp:33,82,174; LinearSearch.cpp:53) unless the sub-pixel extension is on.  So the map crosses PCIe as
// 16-bit integers (the search kernels store them: GenericArgs::out16) whenever the bounds fit, and is widened to the
// caller's CV_32F / CV_64F inside the stage -> caller copy the pool already performs: 2 instead of 4 / 8 bytes per
// pixel on the bus (config 2, CV_64F: 3 MB instead of 12), exact.  Maps that are not integers (sub-pixel) or that
// other kernels read back (smoothFactor, varBlock) cross as float32; doubles never cross.

struct HostBuf { // pinned host memory of the library's own (hipHostMalloc), freed with its owner
    uint8_t *p = nullptr;
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
};

hipError_t host_ensure(HostBuf &b, size_t bytes);

// Is an image worth copying as one linear span, row padding included?  Yes unless it is a narrow
// cut out of a much wider image AND big (the per-row path costs ~15 us per row).
bool linear_span(const ws_image *im);

enum Wire { kWireSame = 0, kWireI16 = 1, kWireF32 = 2 }; // what sits in the stage: the caller's own bytes, int16, float32

// One caller buffer for the duration of a call (or of a batch): how its bytes cross.
struct HostSpan {
    // (ws_last_host_paths reports these values; 1 was a range this library registered itself, rounds 2-3)
    enum How { kUnused = 0, kCallerPinned = 2, kStaged = 3 };
    uint8_t *p = nullptr;
    size_t n = 0;
    How how = kUnused;
    HostBuf *stage = nullptr; // where its bytes cross if they cannot cross directly (set by the call site, always)
    // a download that went to the stage: `rows` rows of `row_elems` elements, dense in the stage from byte stage_off on
    // in wire format, to the caller's buffer from byte host_off on, rows host_pitch bytes apart, in elements of esz bytes
    struct Seg { size_t stage_off, host_off, row_elems, rows, host_pitch; int wire; int esz; };
    std::vector<Seg> down;    // handed to the caller by spans_finish / span_scatter_seg
};

// A caller buffer of `rows` rows of `row_bytes`, `pitch` bytes apart, crossing through `stage` when it must.
inline void span_set(HostSpan &sp, const void *p, size_t pitch, size_t row_bytes, size_t rows, HostBuf *stage)
{
    sp.p = static_cast<uint8_t *>(const_cast<void *>(p));
    sp.n = pitch * (rows - 1) + row_bytes;
    sp.stage = stage;
}

// Classify the buffers of one call.  Spans with p == nullptr or n == 0 stay kUnused.
void spans_attach(HostSpan *sp, int count);

// bytes [off, off + bytes) of the caller's buffer -> device
hipError_t span_upload(HostSpan &sp, size_t off, void *dev, size_t bytes, hipStream_t s);
// rows of `row_bytes`, `pitch` bytes apart in the caller's buffer from byte `off` on -> dense rows on the device
hipError_t span_upload_rows(HostSpan &sp, size_t off, size_t pitch, void *dev, size_t row_bytes, size_t rows, hipStream_t s);

// `rows` dense rows of `row_elems` elements on the device, in wire format -> the caller's buffer from ELEMENT `off` on,
// rows `pitch` elements apart, elements of esz bytes.  A wire format other than the caller's own always goes through
// the stage (the widening is the stage -> caller copy), whatever kind of memory the caller's buffer is.
hipError_t span_download(HostSpan &sp, size_t off, size_t pitch, const void *dev, size_t row_elems, size_t rows, int wire, int esz, hipStream_t s);
// the same for plain bytes (the consumers' buffers): offsets, pitch and row length in bytes
hipError_t span_download_bytes(HostSpan &sp, size_t off, size_t pitch, const void *dev, size_t row_bytes, size_t rows, hipStream_t s);

// Hand a staged download to the caller (the copy of this segment into the stage is through).
void span_scatter_seg(HostSpan &sp, HostSpan::Seg &g);
void span_scatter(HostSpan &sp); // (the copies into the stage are through: the caller of this has synchronised)
// Hand staged downloads to the caller.  ONLY after every stream that carried a copy of these spans is idle.
void spans_finish(HostSpan *sp, int count);

// A caller's image goes up as one linear copy, row padding included (the kernels take any row stride): a 2-D copy
// whose row length is not a multiple of 4 bytes -- 3 * width for most widths -- falls to a per-row path in the runtime
// (measured: 15 ms instead of 0.2 ms for a 1482 x 994 image).  Only a big image cut out of a much wider one
// (linear_span) has its rows gathered into `stage` and goes up dense.
// image_span: fills `sp` for the first kind (left unused for gathered rows) and returns the bytes the image takes on
// the device.  Call it before spans_attach.
size_t image_span(HostSpan &sp, const ws_image *im, HostBuf *stage);
// upload_image: the image -> `dev` (image_span's bytes) on `s`; `*dev_im` is the image as the device holds it.
hipError_t upload_image(HostSpan &sp, const ws_image *im, uint8_t *dev, hipStream_t s, ws_image *dev_im);

} // namespace wsamd
#pragma GCC visibility pop
