// Test driver for BlockSearch::computeDisparityMapsCheckedSGM of the C++ facade
// (stereo_reconstruction_amd/host/window_search.hpp): reads two raw BGR images; writes, as raw doubles, the checked left
// and right maps with the left base, then with the right base and a uniqueness ratio on its winner.
// usage: pair_driver left.raw w1 h1 right.raw w2 h2 bs minD maxD P1 P2 paths maxDiff fill ratio out.raw
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "stereo_reconstruction_amd/host/window_search.hpp"

static std::vector<uint8_t> slurp(const char *path, size_t n)
{
    std::vector<uint8_t> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), 1, n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 17) { fprintf(stderr, "bad usage\n"); return 2; }
    const int w1 = atoi(argv[2]), h1 = atoi(argv[3]), w2 = atoi(argv[5]), h2 = atoi(argv[6]);
    const int bs = atoi(argv[7]), minD = atoi(argv[8]), maxD = atoi(argv[9]);
    const int p1 = atoi(argv[10]), p2 = atoi(argv[11]), paths = atoi(argv[12]);
    const float maxDiff = (float)atof(argv[13]);
    const bool fill = atoi(argv[14]) != 0;
    const int ratio = atoi(argv[15]);
    std::vector<uint8_t> l = slurp(argv[1], (size_t)w1 * h1 * 3), r = slurp(argv[4], (size_t)w2 * h2 * 3);
    try {
        wsamd::BlockSearch search(wsamd::view(l.data(), h1, w1), wsamd::view(r.data(), h2, w2), bs, minD, maxD);
        const std::pair<wsamd::MatF64, wsamd::MatF64> a = search.computeDisparityMapsCheckedSGM(p1, p2, paths, maxDiff, fill);
        const std::pair<wsamd::MatF64, wsamd::MatF64> b = search.computeDisparityMapsCheckedSGM(p1, p2, paths, maxDiff, fill, ratio, false);
        FILE *f = fopen(argv[16], "wb");
        if (!f) return 2;
        for (const wsamd::MatF64 *m : {&a.first, &a.second, &b.first, &b.second}) fwrite(m->ptr(), sizeof(double), (size_t)m->rows * m->cols, f);
        fclose(f);
    } catch (const wsamd::Error &e) {
        fprintf(stderr, "wsamd::Error %d: %s\n", e.code(), e.what());
        return 3;
    }
    return 0;
}
