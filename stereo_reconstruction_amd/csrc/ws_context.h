// ws_context.h -- the context behind the C-ABI's opaque ws_context, for the sources that implement its entry points
// (ws_capi.cpp, ws_lr.cpp, ws_speckle.cpp, ws_sgm.cpp), and what those share: the counter pair behind ws_last_*_counts,
// the frame of a synchronous host call on a pair of images (PairHostCall) and the epilogue of every synchronous host
// call.
#pragma once

#include "ws_capi_internal.h"
#include "ws_search.h"
#include "ws_staging.h"

#include <initializer_list>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace wsamd {

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

// Two unsigned long long that come down behind a call, for ws_last_*_counts: their place on the device (behind the
// kernel's own slot words, if it has any), the pinned host copy, and whether a call has sent them on their way.
struct CountPair {
    DevBuf dev;
    HostBuf host;
    bool ran = false; // a call was enqueued: host holds (or will hold) its counts
    static constexpr size_t kBytes = 2 * sizeof(unsigned long long);
    // room for slot_bytes of the kernel's own in front of the pair, and the host copy's
    int reserve(std::string *err, size_t slot_bytes)
    {
        if (const int rc = ensure(err, dev, slot_bytes + kBytes); rc != WS_OK) return rc;
        WS_HIP(err, host_ensure(host, kBytes));
        return WS_OK;
    }
    // the pair at `sums` (in dev) -> host, on s, behind the kernels that write it: the end of a call's enqueue
    int fetch(std::string *err, const unsigned long long *sums, hipStream_t s)
    {
        WS_HIP(err, hipMemcpyAsync(host.p, sums, kBytes, hipMemcpyDeviceToHost, s));
        ran = true;
        return WS_OK;
    }
};

// The left-right check's device memory (ws_lr.cpp): the two raw maps of ws_search_lr_*, the per-pixel states the fill
// reads, and the failure counters that ws_last_lr_counts reads.  Shared by every check of the context, under its lease.
struct LrState {
    ScratchLease lease;
    DevBuf raw;       // ws_search_lr_*: the left view's map, then the right view's (float32, dense)
    DevBuf states;    // one byte per pixel of both maps (kLrEmpty / kLrPassed / kLrFailed)
    CountPair counts; // the check kernel's failure counters (lr_slot_words()), then their sums: left map, right map
};

// The speckle filter's device memory (ws_speckle.cpp): the four int planes of the labelling, the counters, their sums on
// the way to the host.  Shared by every filter of the context, under its lease.
struct SpeckleState {
    ScratchLease lease;
    DevBuf planes;    // label, parent, count, local: w*h ints each (SpeckleArgs)
    CountPair counts; // speckle_slot_words() counters, then their sums: pixels set, regions removed
};

// Semi-global matching's device memory (ws_sgm.cpp): the candidate intervals, the cost plane and the path sums of one
// call, grown to exactly what the call needs.  Shared by every SGM call of the context, under its lease; the searches'
// own scratch (Searcher) is apart from it.  The uniqueness calls (ws_search_unique_*) are SGM calls in this respect: the
// same scratch, the same lease, and their two counters beside it.
struct SgmState {
    ScratchLease lease;
    DevBuf scratch;
    CountPair counts; // ws_search_unique_*: {failed nodes, nodes}, zeroed on the stream before the winner kernel
};

} // namespace wsamd
#pragma GCC visibility pop

struct ws_context {
    int device = 0;
    int num_cus = 256; // the device's (the consumers' grids; a copy in the Searcher plans the searches)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // ws_timer_begin / ws_timer_end
    wsamd::Searcher searcher;                       // what only the searches touch (ws_search.h)
    wsamd::SgmState sgm;                            // semi-global matching (ws_sgm.cpp)
    wsamd::DevBuf d_left, d_right, d_out, d_out64 /* the consumers' scratch */, d_out16;
    wsamd::DevBuf d_rect_left, d_rect_right; // ws_search_unrectified_host: the rectified images
    wsamd::DevBuf d_mesh, d_mesh_text;       // the mesh text (ws_mesh.hip): per-workgroup sums / offsets and the file's bytes
    wsamd::HostBuf h_mesh[2];                // ... which come down through these two pinned chunks (kMeshChunk each)
    hipEvent_t ev_mesh[2] = {};       // a chunk has landed in h_mesh[i]
    wsamd::Job jobs[2];             // ws_enqueue_host alternates between two slots
    int job_next = 0;
    hipStream_t copy_stream = nullptr; // host <-> device copies of the batched path, beside the searches
    hipStream_t down_stream = nullptr; // ws_search_host in bands: maps go down here while images still come up on copy_stream
    static constexpr int kMaxBands = 8;
    hipEvent_t ev_band_up[kMaxBands] = {}, ev_band_done[kMaxBands] = {}, ev_band_down[kMaxBands] = {};
    wsamd::HostBuf status_page;               // 64 mapped pinned bytes: the words below
    unsigned int *status_host = nullptr, *status_dev = nullptr; // mapped pinned words the kernels flag trouble in (word 0: ws_smooth_left_bands_kernel gave up; word 1: the integer box filter met a value it cannot carry)
    wsamd::DevBuf d_flag;                     // 256 bytes: word 0 = the integer box filter met a value it cannot carry
    int last_outliers_path = 0;        // ws_last_outliers_path
    wsamd::OutlierForms last_outliers_forms[2]; // ws_last_outliers_forms: what the integer / the double launcher launched
    int last_how[3] = {0, 0, 0};       // ws_last_host_paths: how the last host call's left / right / out bytes crossed
    int last_wire = 0;                 // ... and the wire format of its map (ws_last_wire_format)
    std::vector<wsamd::HostSpan> batch_spans; // caller buffers of the pairs enqueued since the last ws_wait (released there)
    wsamd::HostBuf h_left, h_right, h_out;    // ws_search_host: stages (HostSpan), or gathered rows of cut-out images (image_span)
    wsamd::HostBuf h_aux[2];                  // stages of the consumers' further buffers
    int host_bands = -1;               // ws_set_host_bands: 0 = never split, -1 = automatic
    wsamd::LrState lr;                        // the left-right check (ws_lr.cpp)
    wsamd::SpeckleState speckle;              // the speckle filter (ws_speckle.cpp)
    std::string err;
};

#pragma GCC visibility push(hidden)
namespace wsamd {

// What the kernels flagged since the last check (the streams that carried them are idle: the caller synchronised).
int check_device_status(ws_context *ctx);
// The end of a synchronous host call: the streams idle (after an error too: nothing may still be copying when the spans are
// released), staged downloads handed over -- or dropped if the call or a stream failed -- and a stream's error reported.
int finish_host_call(ws_context *ctx, int rc, HostSpan *sp, int count, std::initializer_list<hipStream_t> streams, const char *what);

// A synchronous host call on a pair of images, on the context's stream: open(), the caller's output spans from sp[2] on
// and spans_attach, upload(), the call's own work and downloads, close().
struct PairHostCall {
    ws_context *ctx;
    const ws_image *left, *right;
    hipStream_t s;  // the context's stream
    HostSpan sp[5]; // the caller's buffers for the duration of the call: the images, then the outputs
    ws_image dl, dr; // the images as the device holds them (upload)
    PairHostCall(ws_context *c, const ws_image *l, const ws_image *r) : ctx(c), left(l), right(r), s(c->stream) {}
    int open();   // sp[0], sp[1] and room in d_left / d_right
    int upload(); // both images -> d_left / d_right on s
    // How the images and the map crossed and the map's wire format for ws_last_host_paths / ws_last_wire_format
    // (wire < 0: the call leaves them alone), then finish_host_call on `streams` (none: s) with the first `count`
    // spans, then -- for a call that ran the search dispatch (device_status) -- what its kernels flagged.
    int close(int rc, int count, int wire, bool device_status, const char *what, std::initializer_list<hipStream_t> streams = {});
};

// What ws_lr.cpp shares with ws_pair.cpp, all under the context's left-right lease.  check_lr: the refusals of a
// ws_lr_params.  lr_maps: two maps in, two out, strides in floats.  lr_maps_scratch: LrState::raw as both raw maps
// (dense), then (checked_too) both checked maps; offsets in floats.  enqueue_check: zeroed counters, the check kernel,
// the fill if asked for, and the counts on their way to the host, all on s.
int check_lr(std::string *err, const ws_lr_params *lr);
LrMaps lr_maps(const float *l, int lw, int lh, int lstride, const float *r, int rw, int rh, int rstride, float *ol, int olstride,
               float *orr, int orstride);
int lr_maps_scratch(ws_context *ctx, size_t n_left, size_t n_right, int checked_too, float **base, size_t off[4]);
int enqueue_check(ws_context *ctx, LrMaps m, const ws_lr_params *lr, hipStream_t s);

// ws_last_*_counts: the pair of the last call under `lease` to out, once that call is through; `none`: the refusal if no
// call has run.
int read_counts(ws_context *ctx, CountPair &c, ScratchLease &lease, const char *none, unsigned long long out[2]);

} // namespace wsamd
#pragma GCC visibility pop
