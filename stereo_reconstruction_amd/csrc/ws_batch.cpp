// ws_batch.cpp -- ws_batch_* of include/ws_stereo.h: many independent pairs dealt to several contexts (workers), each
// driven by a host thread of its own.  The assignment and the queues are ws_batch_core.h; a worker's items go through
// the batched host path of its context (ws_enqueue_host, or its row-band form for bands) and end with ws_wait.  No
// kernel of its own: every search is the one ws_search_host runs.
#include "../../include/ws_stereo.h"
#include "ws_batch_core.h"
#include "ws_capi_internal.h"

#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

struct ws_batch {
    std::vector<int> devices;
    std::vector<ws_context *> ctx; // one per worker
    std::string err;
};

namespace {

thread_local std::string g_batch_error; // ws_batch_last_error(NULL)

int fail(ws_batch *b, int code, const char *fmt, ...)
{
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (b ? b->err : g_batch_error) = buf;
    return code;
}

long long job_nd(const ws_params &p)
{
    return p.view == WS_VIEW_LEFT ? (long long)p.max_disparity
         : p.view == WS_VIEW_RIGHT ? (long long)p.max_disparity - p.min_disparity
                                   : (long long)p.linear_range;
}

// ws_search_host's own test for cutting a call into bands (ws_capi.cpp): no raster dependency, no varBlock growth, no
// census cost (its descriptors look ry rows beyond the window's halo); sharding.can_band restates it
bool band_ok(const ws_job &j)
{
    const bool census = j.params.cost == WS_COST_CENSUS_5X5 || j.params.cost == WS_COST_CENSUS_9X7;
    return (j.params.view == WS_VIEW_LEFT || j.params.view == WS_VIEW_RIGHT) && j.params.smooth_factor == 1.0 &&
           !j.params.var_block && !census && j.left.height == j.right.height;
}

// The checks of one job: its parameters and images as ws_validate checks them, and (outputs) its map buffer as
// ws_enqueue_host does.  The message names the job.
int check_job(ws_batch *b, const ws_job &j, int i, bool outputs)
{
    const int rc = ws_validate(&j.params, &j.left, &j.right);
    if (rc != WS_OK) return fail(b, rc, "job %d: %s", i, ws_last_error(nullptr));
    if (!outputs) return WS_OK;
    if (!j.out || (j.out_dtype != WS_OUT_F32 && j.out_dtype != WS_OUT_F64)) return fail(b, WS_ERR_ARG, "job %d: bad output", i);
    int ow, oh;
    wsamd::map_dims(&j.params, &j.left, &j.right, &ow, &oh);
    if (j.out_stride < ow) return fail(b, WS_ERR_ARG, "job %d: out_stride %d < width %d", i, j.out_stride, ow);
    return WS_OK;
}

int make_plan(ws_batch *b, const ws_job *jobs, int n_jobs, int n_workers, int bands, int min_rows,
              std::vector<wsbatch::Item> *items, bool *banded)
{
    if (n_jobs < 0 || (n_jobs > 0 && !jobs) || n_workers < 1 || (bands != 0 && bands != 1) || min_rows < 1)
        return fail(b, WS_ERR_ARG, "bad arguments (n_jobs %d, n_workers %d, bands %d, min_rows %d)", n_jobs, n_workers, bands, min_rows);
    std::vector<wsbatch::Shape> shapes;
    bool can = bands == 1;
    for (int i = 0; i < n_jobs; ++i) {
        int ow, oh;
        wsamd::map_dims(&jobs[i].params, &jobs[i].left, &jobs[i].right, &ow, &oh);
        shapes.push_back({ow, oh, job_nd(jobs[i].params)});
        can = can && band_ok(jobs[i]) && jobs[i].params.block_size == jobs[0].params.block_size &&
              shapes.back().nd == shapes[0].nd && shapes[0].nd >= 1;
    }
    *banded = can;
    *items = wsbatch::plan(shapes, n_workers, can, n_jobs ? jobs[0].params.block_size : 1, min_rows);
    return WS_OK;
}

} // namespace

extern "C" {

int ws_batch_create(const int *devices, int n_workers, ws_batch **out)
{
    if (!out) return fail(nullptr, WS_ERR_ARG, "null output");
    *out = nullptr;
    std::vector<int> devs;
    if (devices) {
        if (n_workers < 1) return fail(nullptr, WS_ERR_ARG, "n_workers %d < 1", n_workers);
        devs.assign(devices, devices + n_workers);
    } else {
        const int n = ws_device_count();
        if (n < 1) return fail(nullptr, WS_ERR_HIP, "no HIP device available: this library has no CPU path");
        for (int d = 0; d < n; ++d) devs.push_back(d);
    }
    ws_batch *b = new (std::nothrow) ws_batch();
    if (!b) return fail(nullptr, WS_ERR_NOMEM, "out of host memory");
    b->devices = devs;
    // (created here, on the calling thread: a failure's text is this thread's ws_last_error(NULL))
    for (size_t w = 0; w < devs.size(); ++w) {
        ws_context *c = nullptr;
        const int rc = ws_create(devs[w], &c);
        if (rc != WS_OK) {
            fail(nullptr, rc, "worker %d (device %d): %s", (int)w, devs[w], ws_last_error(nullptr));
            ws_batch_destroy(b);
            return rc;
        }
        b->ctx.push_back(c);
    }
    *out = b;
    return WS_OK;
}

void ws_batch_destroy(ws_batch *b)
{
    if (!b) return;
    for (ws_context *c : b->ctx) ws_destroy(c);
    delete b;
}

const char *ws_batch_last_error(const ws_batch *b) { return b ? b->err.c_str() : g_batch_error.c_str(); }

int ws_batch_workers(const ws_batch *b, int *devices, int cap)
{
    if (!b) return 0;
    for (int w = 0; devices && w < cap && w < (int)b->devices.size(); ++w) devices[w] = b->devices[(size_t)w];
    return (int)b->devices.size();
}

int ws_batch_plan(const ws_job *jobs, int n_jobs, int n_workers, int bands, int min_rows, ws_batch_item *items, int cap,
                  int *n_items, int *banded)
{
    if (!n_items || !banded || cap < 0 || (cap > 0 && !items)) return fail(nullptr, WS_ERR_ARG, "null output");
    *n_items = 0;
    *banded = 0;
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(nullptr, WS_ERR_ARG, "bad jobs");
    int rc;
    for (int i = 0; i < n_jobs; ++i)
        if ((rc = check_job(nullptr, jobs[i], i, false)) != WS_OK) return rc;
    std::vector<wsbatch::Item> plan;
    bool b = false;
    if ((rc = make_plan(nullptr, jobs, n_jobs, n_workers, bands, min_rows, &plan, &b)) != WS_OK) return rc;
    *n_items = (int)plan.size();
    *banded = b;
    if ((int)plan.size() > cap) return fail(nullptr, WS_ERR_ARG, "%d items, room for %d", (int)plan.size(), cap);
    for (size_t i = 0; i < plan.size(); ++i) items[i] = {plan[i].job, plan[i].y0, plan[i].y1, plan[i].worker};
    return WS_OK;
}

int ws_batch_search_host(ws_batch *b, ws_job *jobs, int n_jobs, int bands, int min_rows)
{
    if (!b) return WS_ERR_ARG;
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(b, WS_ERR_ARG, "bad jobs");
    // every job is checked before anything starts: one invalid job and nothing is searched, no `out` written
    int rc = WS_OK;
    for (int i = n_jobs - 1; i >= 0; --i) { // (backwards: the lowest-index failure's message is the one that stays)
        const int s = check_job(b, jobs[i], i, true);
        jobs[i].status = s == WS_OK ? WS_JOB_NOT_RUN : s;
        if (s != WS_OK) rc = s;
    }
    if (rc != WS_OK) return rc;
    std::vector<wsbatch::Item> items;
    bool banded = false;
    if ((rc = make_plan(b, jobs, n_jobs, (int)b->ctx.size(), bands, min_rows, &items, &banded)) != WS_OK) return rc;
    auto run_item = [&](int w, const wsbatch::Item &it) -> int {
        const ws_job &j = jobs[it.job];
        int ow, oh;
        wsamd::map_dims(&j.params, &j.left, &j.right, &ow, &oh);
        if (it.y0 == 0 && it.y1 == oh)
            return ws_enqueue_host(b->ctx[(size_t)w], &j.params, &j.left, &j.right, j.out, j.out_stride, j.out_dtype);
        // a row band (equal image heights): the sub-images under its rows and the window's halo
        const int half = (j.params.block_size - 1) / 2;
        const int a = it.y0 - half > 0 ? it.y0 - half : 0, e = it.y1 + half < oh ? it.y1 + half : oh;
        const ws_image l{j.left.data + (size_t)a * j.left.stride, j.left.width, e - a, j.left.stride};
        const ws_image r{j.right.data + (size_t)a * j.right.stride, j.right.width, e - a, j.right.stride};
        const size_t esz = (size_t)wsamd::out_elem_size(j.out_dtype);
        void *out = static_cast<uint8_t *>(j.out) + (size_t)it.y0 * j.out_stride * esz;
        return wsamd::enqueue_host_rows(b->ctx[(size_t)w], &j.params, &l, &r, out, j.out_stride, j.out_dtype, it.y0 - a, it.y1 - it.y0);
    };
    auto finish = [&](int w) -> int { return ws_wait(b->ctx[(size_t)w]); };
    std::vector<int> status;
    wsbatch::run(items, (int)b->ctx.size(), run_item, finish, status);
    std::vector<int> per_job((size_t)n_jobs);
    int first = -1;
    rc = wsbatch::job_status(items, status, n_jobs, per_job.data(), &first);
    for (int i = 0; i < n_jobs; ++i) jobs[i].status = per_job[(size_t)i];
    if (rc != WS_OK) {
        int worker = 0; // the worker of the job's first failed item: its context holds the message
        for (size_t i = 0; i < items.size(); ++i)
            if (items[i].job == first && status[i] < 0) {
                worker = items[i].worker;
                break;
            }
        return fail(b, rc, "job %d (worker %d, device %d): %s", first, worker, b->devices[(size_t)worker], ws_last_error(b->ctx[(size_t)worker]));
    }
    b->err.clear();
    return WS_OK;
}

} // extern "C"
