// ws_batch_core.h -- the scheduling core of ws_batch_* (include/ws_stereo.h, "many pairs over the devices of a node"):
// which worker searches which rows of which pair, and the per-worker queues that run them.  No HIP in here: the C-ABI
// (ws_batch.cpp) drives it with real contexts, tests/cxx/batch_core_check.cpp with fake workers under ThreadSanitizer.
//
// The two assignments restate stereo_reconstruction_amd/sharding.py exactly -- the same items, the same workers --
// so that a C++ caller and bench.py's launcher deal a batch alike:
//   lpt_assign: whole pairs, longest first, each to the least loaded worker (ties: the lower index);
//   band_items: the pairs' rows laid end to end and cut into `world` runs of equal weight, bands of >= min_rows rows.
// Python evaluates those in doubles in a fixed order; so does this (round() is half-to-even: nearbyint).
#pragma once

#include <math.h>

#include <algorithm>
#include <exception>
#include <new>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/ws_stereo.h"

namespace wsbatch {

struct Item { // map rows [y0, y1) of job `job`, searched by worker `worker`
    int job, y0, y1, worker;
};

struct Shape { // a job's map: out_w x out_h, nd disparities per pixel
    int w, h;
    long long nd;
};

// sharding.lpt_assign(costs, world): shards[r] = the job indices of worker r, ascending.
inline std::vector<std::vector<int>> lpt_assign(const std::vector<long long> &costs, int world)
{
    std::vector<int> order(costs.size());
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return costs[a] != costs[b] ? costs[a] > costs[b] : a < b; });
    std::vector<double> load((size_t)world, 0.0);
    std::vector<std::vector<int>> shards((size_t)world);
    for (int i : order) {
        int r = 0;
        for (int k = 1; k < world; ++k)
            if (load[k] < load[r]) r = k; // (strict: the lower index keeps a tie)
        shards[r].push_back(i);
        load[r] += (double)costs[i];
    }
    for (std::vector<int> &s : shards) std::sort(s.begin(), s.end());
    return shards;
}

// sharding.band_items(shapes, max_d, world, block_size, min_rows): items grouped by worker, in the order the cut made
// them (Item::worker = the rank).  shapes: (w, h) per pair; every pair's rows weigh w * max_d each.
inline std::vector<Item> band_items(const std::vector<Shape> &shapes, long long max_d, int world, int block_size, int min_rows)
{
    const int half = (block_size - 1) / 2;
    const int n = (int)shapes.size();
    const double md = (double)max_d;
    auto cost = [&](const Item &it) {
        const Shape &s = shapes[(size_t)it.job];
        return (double)(std::min(s.h, it.y1 + half) - std::max(0, it.y0 - half)) * s.w * md;
    };
    auto cut = [&](const std::vector<int> &order) {
        std::vector<std::vector<Item>> per_rank((size_t)world);
        long long area = 0;
        for (int i : order) area += (long long)shapes[(size_t)i].w * shapes[(size_t)i].h;
        double remaining = (double)area * md;
        int pos = 0, y = 0;
        for (int r = 0; r < world; ++r) {
            const double target = remaining / (double)(world - r);
            double got = 0.0;
            const bool last = r == world - 1;
            while (pos < n) {
                const int i = order[(size_t)pos];
                const int w = shapes[(size_t)i].w, h = shapes[(size_t)i].h;
                const double rest = (double)(h - y) * w * md;
                if (last || got + rest <= target) {
                    if (h > y) per_rank[(size_t)r].push_back({i, y, h, r});
                    got += rest;
                    pos += 1;
                    y = 0;
                    continue;
                }
                // the ideal cut lies inside this pair
                int yc = y + (int)nearbyint((target - got) / (double)((long long)w * max_d));
                const int lo = y + min_rows, hi = h - min_rows; // both bands keep min_rows rows
                if (lo > hi) {                                  // the rest cannot be cut: all of it or none of it
                    yc = (target - got) * 2 >= rest ? h : y;
                } else if (yc - y < min_rows) {
                    yc = (yc - y) * 2 < min_rows ? y : lo;
                } else if (h - yc < min_rows) {
                    yc = (h - yc) * 2 < min_rows ? h : hi;
                }
                if (yc > y) {
                    per_rank[(size_t)r].push_back({i, y, yc, r});
                    got += (double)(yc - y) * w * md;
                }
                if (yc >= h) {
                    pos += 1;
                    y = 0;
                } else {
                    y = yc;
                }
                break;
            }
            remaining -= got;
        }
        return per_rank;
    };
    // the orders tried, in Python's sequence: rotations of the given order, largest first, smallest first
    std::vector<std::vector<int>> orders;
    for (int k = 0; k < std::max(n, 1); ++k) {
        std::vector<int> o;
        for (int i = k; i < n; ++i) o.push_back(i);
        for (int i = 0; i < k && i < n; ++i) o.push_back(i);
        orders.push_back(o);
    }
    std::vector<int> by_cost((size_t)n);
    std::iota(by_cost.begin(), by_cost.end(), 0);
    auto area = [&](int i) { return (long long)shapes[(size_t)i].w * shapes[(size_t)i].h; };
    std::sort(by_cost.begin(), by_cost.end(), [&](int a, int b) { return area(a) != area(b) ? area(a) > area(b) : a < b; });
    orders.push_back(by_cost);
    orders.push_back(std::vector<int>(by_cost.rbegin(), by_cost.rend()));
    std::vector<std::vector<Item>> best;
    double best_load = 0.0;
    bool have = false;
    for (const std::vector<int> &o : orders) {
        std::vector<std::vector<Item>> per_rank = cut(o);
        double load = 0.0;
        for (size_t r = 0; r < per_rank.size(); ++r) {
            double s = 0.0;
            for (const Item &it : per_rank[r]) s += cost(it);
            if (r == 0 || s > load) load = s;
        }
        if (!have || load < best_load) {
            best = std::move(per_rank);
            best_load = load;
            have = true;
        }
    }
    std::vector<Item> items;
    for (const std::vector<Item> &v : best) items.insert(items.end(), v.begin(), v.end());
    return items;
}

// What a batch call would run.  bandable: every job passed the per-job band test and all share block_size and nd (the
// caller's checks); banded then cuts row bands, else whole pairs by LPT with cost w * h * nd.
inline std::vector<Item> plan(const std::vector<Shape> &jobs, int world, bool bandable, int block_size, int min_rows)
{
    if (bandable) return band_items(jobs, jobs.empty() ? 1 : jobs[0].nd, world, block_size, min_rows);
    std::vector<long long> costs;
    for (const Shape &s : jobs) costs.push_back((long long)s.w * s.h * s.nd);
    std::vector<Item> items;
    const std::vector<std::vector<int>> shards = lpt_assign(costs, world);
    for (int r = 0; r < world; ++r)
        for (int j : shards[(size_t)r]) items.push_back({j, 0, jobs[(size_t)j].h, r});
    return items;
}

// Run `items` on `world` workers, one host thread each (worker 0 on the calling thread).  A worker runs its own items in
// order: run_item(worker, item) -> WS_OK or an error.  After its first error it runs nothing more: its remaining items
// become WS_JOB_NOT_RUN.  finish(worker) -> status is then called once per worker whatever happened (it drains the work
// the worker still has in flight); if it fails, every item of that worker that had returned WS_OK takes its status too
// (that item's result may not have landed).  status[i] receives item i's outcome.  An exception out of a callable counts
// as WS_ERR_NOMEM.
template <class RunItem, class Finish>
void run(const std::vector<Item> &items, int world, RunItem run_item, Finish finish, std::vector<int> &status)
{
    status.assign(items.size(), WS_JOB_NOT_RUN);
    std::vector<std::vector<int>> queue((size_t)world);
    for (size_t i = 0; i < items.size(); ++i) queue[(size_t)items[i].worker].push_back((int)i);
    auto worker = [&](int w) {
        int err = WS_OK;
        for (int i : queue[(size_t)w]) {
            if (err != WS_OK) break; // (status stays WS_JOB_NOT_RUN)
            int rc;
            try { rc = run_item(w, items[(size_t)i]); } catch (...) { rc = WS_ERR_NOMEM; }
            status[(size_t)i] = rc;
            err = rc;
        }
        int f;
        try { f = finish(w); } catch (...) { f = WS_ERR_NOMEM; }
        if (f != WS_OK)
            for (int i : queue[(size_t)w])
                if (status[(size_t)i] == WS_OK) status[(size_t)i] = f;
    };
    std::vector<std::thread> threads;
    std::vector<int> inline_workers; // (workers no thread could be started for run here, after worker 0)
    for (int w = 1; w < world; ++w) {
        if (queue[(size_t)w].empty()) continue;
        try { threads.emplace_back(worker, w); } catch (...) { inline_workers.push_back(w); }
    }
    if (world > 0 && !queue[0].empty()) worker(0);
    for (int w : inline_workers) worker(w);
    for (std::thread &t : threads) t.join();
}

// Per job: WS_OK if all its items succeeded, else the first error among its items (in item order), else
// WS_JOB_NOT_RUN.  Returns the status of the lowest-index job that failed with an error (WS_OK if none did), and that
// job's index in *first (-1 if none).
inline int job_status(const std::vector<Item> &items, const std::vector<int> &status, int n_jobs, int *out, int *first)
{
    for (int j = 0; j < n_jobs; ++j) out[j] = WS_OK;
    for (size_t i = 0; i < items.size(); ++i) {
        int &s = out[items[i].job];
        if (status[i] < 0 && s >= 0) s = status[i];
        else if (status[i] == WS_JOB_NOT_RUN && s == WS_OK) s = WS_JOB_NOT_RUN;
    }
    *first = -1;
    for (int j = 0; j < n_jobs; ++j)
        if (out[j] < 0) {
            *first = j;
            return out[j];
        }
    return WS_OK;
}

} // namespace wsbatch
