// Test driver for wsamd::BatchSearch (stereo_reconstruction_amd/host/window_search.hpp): reads a batch description,
// runs it once through BatchSearch::run and once pair by pair through ws_search_host on one context, writes the batch's
// maps (raw doubles) and prints "same" if every map is bit-identical to the one-context map.
// usage: batch_driver spec.txt
//   line 1: bands min_rows device...            (no device: every device)
//   then one line per pair: left.raw right.raw width height view(left|right) bs minD maxD out.raw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "stereo_reconstruction_amd/host/window_search.hpp"

static std::vector<uint8_t> slurp(const std::string &path, size_t n)
{
    std::vector<uint8_t> v(n);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(v.data(), 1, n, f) != n) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "bad usage\n"); return 2; }
    std::ifstream spec(argv[1]);
    std::string line;
    std::getline(spec, line);
    std::istringstream head(line);
    int bands = 0, minRows = 0, d;
    head >> bands >> minRows;
    std::vector<int> devices;
    while (head >> d) devices.push_back(d);
    std::vector<std::vector<uint8_t>> images;
    std::vector<wsamd::BatchSearch::Job> jobs;
    std::vector<std::string> outs;
    while (std::getline(spec, line)) {
        std::istringstream in(line);
        std::string lp, rp, view, op;
        int w, h, bs, minD, maxD;
        if (!(in >> lp >> rp >> w >> h >> view >> bs >> minD >> maxD >> op)) continue;
        images.push_back(slurp(lp, (size_t)w * h * 3));
        images.push_back(slurp(rp, (size_t)w * h * 3));
        outs.push_back(op);
    }
    // (the image buffers are all read before any view of them is taken: `images` no longer moves)
    {
        std::ifstream again(argv[1]);
        std::getline(again, line);
        size_t k = 0;
        while (std::getline(again, line)) {
            std::istringstream in(line);
            std::string lp, rp, view, op;
            int w, h, bs, minD, maxD;
            if (!(in >> lp >> rp >> w >> h >> view >> bs >> minD >> maxD >> op)) continue;
            wsamd::BatchSearch::Job j;
            j.params = wsamd::BatchSearch::params(view == "left" ? WS_VIEW_LEFT : WS_VIEW_RIGHT, bs, minD, maxD, 1.0);
            j.left = wsamd::view(images[2 * k].data(), h, w);
            j.right = wsamd::view(images[2 * k + 1].data(), h, w);
            jobs.push_back(j);
            ++k;
        }
    }
    try {
        wsamd::BatchSearch batch(devices);
        std::vector<wsamd::MatF64> maps = batch.run(jobs, bands != 0, minRows);
        wsamd::Device one(0);
        bool same = maps.size() == jobs.size();
        for (size_t i = 0; i < jobs.size() && same; ++i) {
            wsamd::MatF64 want(maps[i].rows, maps[i].cols);
            const ws_image l = wsamd::detail::to_c(jobs[i].left), r = wsamd::detail::to_c(jobs[i].right);
            const int rc = ws_search_host(one.get(), &jobs[i].params, &l, &r, want.ptr(), want.cols, WS_OUT_F64);
            if (rc != WS_OK) throw wsamd::Error(rc, ws_last_error(one.get()));
            same = memcmp(want.ptr(), maps[i].ptr(), sizeof(double) * want.rows * want.cols) == 0;
            FILE *f = fopen(outs[i].c_str(), "wb");
            if (!f || fwrite(maps[i].ptr(), sizeof(double), (size_t)maps[i].rows * maps[i].cols, f) != (size_t)maps[i].rows * maps[i].cols)
                return 3;
            fclose(f);
        }
        printf("%s workers=%d pairs=%zu\n", same ? "same" : "DIFFERENT", batch.workers(), jobs.size());
        return same ? 0 : 4;
    } catch (const wsamd::Error &e) {
        fprintf(stderr, "wsamd::Error %d: %s\n", e.code(), e.what());
        return 10 - e.code();
    }
}
