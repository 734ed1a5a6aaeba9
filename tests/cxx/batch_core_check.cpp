// Drives the scheduling core of ws_batch_* (stereo_reconstruction_amd/csrc/ws_batch_core.h) with fake workers -- no
// HIP, no device -- under ThreadSanitizer (tests/test_batch_core.py builds it with g++ -fsanitize=thread).  Prints
// "batch core ok" when every check holds; any failed check prints its line and exits 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include "stereo_reconstruction_amd/csrc/ws_batch_core.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

using wsbatch::Item;

static void spin_us(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

// workers of uneven speed: every item runs exactly once, on its own worker; finish once per busy worker
static void uneven_speeds()
{
    const int world = 5;
    std::vector<Item> items;
    for (int i = 0; i < 60; ++i) items.push_back({i % 17, 0, 1, (i * 7) % world});
    std::vector<std::atomic<int>> runs(items.size());
    std::vector<std::atomic<int>> finishes(world);
    std::vector<int> status;
    wsbatch::run(
        items, world,
        [&](int w, const Item &it) {
            CHECK(it.worker == w);
            runs[(size_t)(&it - items.data())].fetch_add(1);
            spin_us(50 * (w + 1) * (w + 1)); // worker 4 is 25 x slower than worker 0
            return WS_OK;
        },
        [&](int w) {
            finishes[(size_t)w].fetch_add(1);
            return WS_OK;
        },
        status);
    for (size_t i = 0; i < items.size(); ++i) CHECK(runs[i].load() == 1 && status[i] == WS_OK);
    for (int w = 0; w < world; ++w) CHECK(finishes[(size_t)w].load() == 1);
    std::vector<int> per_job(17);
    int first = 7;
    CHECK(wsbatch::job_status(items, status, 17, per_job.data(), &first) == WS_OK && first == -1);
    for (int s : per_job) CHECK(s == WS_OK);
}

// a worker that fails mid-queue stops; its later items are NOT_RUN and never run; the others finish
static void failing_worker()
{
    const int world = 3;
    // worker 1's queue: jobs 6, 5, 2, 1 -- it fails on job 5; jobs 2 and 1 are then not run
    std::vector<Item> items = {{0, 0, 1, 0}, {6, 0, 1, 1}, {3, 0, 1, 2}, {5, 0, 1, 1}, {4, 0, 1, 0},
                               {2, 0, 1, 1}, {7, 0, 1, 2}, {1, 0, 10, 1}, {1, 10, 20, 0}};
    std::vector<std::atomic<int>> runs(items.size());
    std::vector<std::atomic<int>> finishes(world);
    std::vector<int> status;
    wsbatch::run(
        items, world,
        [&](int w, const Item &it) {
            runs[(size_t)(&it - items.data())].fetch_add(1);
            spin_us(200 * (2 - w));
            return w == 1 && it.job == 5 ? WS_ERR_HIP : WS_OK;
        },
        [&](int w) {
            finishes[(size_t)w].fetch_add(1);
            return WS_OK;
        },
        status);
    const int want_runs[] = {1, 1, 1, 1, 1, 0, 1, 0, 1};
    const int want_status[] = {WS_OK, WS_OK, WS_OK, WS_ERR_HIP, WS_OK, WS_JOB_NOT_RUN, WS_OK, WS_JOB_NOT_RUN, WS_OK};
    for (size_t i = 0; i < items.size(); ++i) CHECK(runs[i].load() == want_runs[i] && status[i] == want_status[i]);
    for (int w = 0; w < world; ++w) CHECK(finishes[(size_t)w].load() == 1); // (also the worker that failed)
    std::vector<int> per_job(8);
    int first = -1;
    // job 1 (a band ran, a band did not) and job 2 are NOT_RUN, job 5 failed: the call's status is job 5's
    CHECK(wsbatch::job_status(items, status, 8, per_job.data(), &first) == WS_ERR_HIP && first == 5);
    const int want_job[] = {WS_OK, WS_JOB_NOT_RUN, WS_JOB_NOT_RUN, WS_OK, WS_OK, WS_ERR_HIP, WS_OK, WS_OK};
    for (int j = 0; j < 8; ++j) CHECK(per_job[(size_t)j] == want_job[j]);
    // two failures: the lower job index decides, whichever worker met its error first
    std::vector<int> st2 = {WS_OK, WS_ERR_NOMEM, WS_OK, WS_OK, WS_ERR_ARG, WS_OK, WS_OK, WS_OK, WS_OK};
    CHECK(wsbatch::job_status(items, st2, 8, per_job.data(), &first) == WS_ERR_ARG && first == 4);
}

// finish failing (the wait of a worker's context): every item of that worker that had succeeded takes its status;
// a throwing item counts as WS_ERR_NOMEM
static void failing_finish_and_throw()
{
    const int world = 4;
    std::vector<Item> items;
    for (int i = 0; i < 24; ++i) items.push_back({i, 0, 1, i % world});
    std::vector<int> status;
    wsbatch::run(
        items, world,
        [&](int w, const Item &it) -> int {
            if (w == 3 && it.job == 15) throw std::bad_alloc();
            return WS_OK;
        },
        [&](int w) { return w == 2 ? WS_ERR_HIP : WS_OK; }, status);
    for (size_t i = 0; i < items.size(); ++i) {
        const int w = items[i].worker, j = items[i].job;
        const int want = w == 2 ? WS_ERR_HIP : w == 3 && j == 15 ? WS_ERR_NOMEM : w == 3 && j > 15 ? WS_JOB_NOT_RUN : WS_OK;
        CHECK(status[i] == want);
    }
}

// the real plan of a trainingH batch over 8 workers: fake workers write their band's rows of a shared map each;
// every row of every pair is written exactly once, and no two workers touch the same row (ThreadSanitizer would see it)
static void bands_cover_every_row_once()
{
    const int shapes[15][2] = {{1436, 992}, {694, 554}, {1318, 994}, {1482, 994}, {1482, 994}, {1414, 962}, {1414, 962}, {1470, 970},
                               {1398, 952}, {1360, 926}, {1362, 924}, {1440, 972}, {1476, 994}, {900, 750}, {1444, 960}};
    std::vector<wsbatch::Shape> jobs;
    for (const auto &s : shapes) jobs.push_back({s[0], s[1], 256});
    for (int world : {1, 2, 3, 8, 40}) {
        const std::vector<Item> items = wsbatch::plan(jobs, world, true, 7, 256);
        std::vector<std::vector<int>> rows(jobs.size());
        for (size_t j = 0; j < jobs.size(); ++j) rows[j].assign((size_t)jobs[j].h, 0);
        std::vector<int> status;
        wsbatch::run(
            items, world,
            [&](int, const Item &it) {
                for (int y = it.y0; y < it.y1; ++y) rows[(size_t)it.job][(size_t)y] += 1;
                return WS_OK;
            },
            [&](int) { return WS_OK; }, status);
        for (size_t j = 0; j < jobs.size(); ++j)
            for (int v : rows[j]) CHECK(v == 1);
        for (const Item &it : items) CHECK(it.y1 - it.y0 >= 256 || (it.y0 == 0 && it.y1 == jobs[(size_t)it.job].h));
        // whole pairs: each job once
        const std::vector<Item> whole = wsbatch::plan(jobs, world, false, 7, 256);
        CHECK(whole.size() == jobs.size());
    }
}

int main()
{
    for (int rep = 0; rep < 3; ++rep) {
        uneven_speeds();
        failing_worker();
        failing_finish_and_throw();
    }
    bands_cover_every_row_once();
    printf("batch core ok\n");
    return 0;
}
