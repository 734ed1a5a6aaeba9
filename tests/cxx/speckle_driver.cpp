// Test driver for wsamd::filterSpeckles of the C++ facade (stereo_reconstruction_amd/host/window_search.hpp): reads a raw
// float32 map, filters it in place with OpenCV's argument order, writes it back out as raw float32.
// usage: speckle_driver map.raw w h newVal maxSpeckleSize maxDiff out.raw
#include <cstdio>
#include <cstdlib>

#include "stereo_reconstruction_amd/host/window_search.hpp"

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "bad usage\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    wsamd::MatF32 map(h, w);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(map.ptr(), sizeof(float), (size_t)w * h, f) != (size_t)w * h) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    try {
        wsamd::filterSpeckles(map, atof(argv[4]), atoi(argv[5]), atof(argv[6]));
    } catch (const wsamd::Error &e) {
        fprintf(stderr, "wsamd::Error %d: %s\n", e.code(), e.what());
        return 3;
    }
    f = fopen(argv[7], "wb");
    if (!f) return 2;
    fwrite(map.ptr(), sizeof(float), (size_t)w * h, f);
    fclose(f);
    return 0;
}
