// mesh_text_check.cpp -- stereo_reconstruction_amd/csrc/ws_text.h against the C library, byte for byte, on the host:
// g_format(f) == snprintf("%g", (double)f) (what `std::ostream << float` writes, the host mesh writer's text) and
// u_format(v) == snprintf("%u" / "%zu", v).
//   mesh_text_check <threads> <random patterns>
// Prints the first mismatches and exits 1 if there is any, else prints what it covered and exits 0.
#include "../../stereo_reconstruction_amd/csrc/ws_text.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

using namespace wsamd::text;

static std::atomic<unsigned long long> g_checked{0}, g_bad{0};
static std::mutex g_print;

static float from_bits(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static bool check_float(float f)
{
    char want[64], got[kMaxG + 4];
    const int wn = snprintf(want, sizeof want, "%g", (double)f);
    const G6 g = g6_decompose(f);
    const int gn = g6_write(g, got);
    const int ln = g6_length(g);
    if (gn == wn && ln == wn && gn <= kMaxG && memcmp(want, got, wn) == 0) return true;
    if (g_bad.fetch_add(1) < 20) {
        uint32_t b;
        memcpy(&b, &f, 4);
        std::lock_guard<std::mutex> lock(g_print);
        fprintf(stderr, "float 0x%08x: want \"%s\" got \"%.*s\" (length %d)\n", b, want, gn, got, ln);
    }
    return false;
}

template <class U> static bool check_unsigned(U v)
{
    char want[32], got[32];
    const int wn = snprintf(want, sizeof want, "%llu", (unsigned long long)v);
    const int gn = u_format(v, got);
    if (gn == wn && u_length(v) == wn && memcmp(want, got, wn) == 0) return true;
    if (g_bad.fetch_add(1) < 20) {
        std::lock_guard<std::mutex> lock(g_print);
        fprintf(stderr, "unsigned %llu: got \"%.*s\"\n", (unsigned long long)v, gn, got);
    }
    return false;
}

// bit patterns [lo, hi) of the float space, split over the threads
static void run_range(uint64_t lo, uint64_t hi, int threads)
{
    std::vector<std::thread> pool;
    const uint64_t step = (hi - lo + threads - 1) / threads;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            unsigned long long n = 0;
            for (uint64_t b = lo + t * step; b < hi && b < lo + (t + 1) * step; ++b, ++n) check_float(from_bits((uint32_t)b));
            g_checked += n;
        });
    for (auto &th : pool) th.join();
}

static uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char **argv)
{
    const int threads = argc > 1 ? atoi(argv[1]) : 4;
    const unsigned long long randoms = argc > 2 ? strtoull(argv[2], nullptr, 10) : 100000000ull;
    if (threads < 1) return 2;

    // 1. every float of the binades that hold the %f / %e switch: 2^-17 .. 2^-13 (1e-5, 1e-4) and 2^16 .. 2^23 (1e5, 1e6, 1e7)
    for (int p : {-17, -16, -15, -14, -13, 16, 17, 18, 19, 20, 21, 22, 23}) {
        const uint64_t lo = (uint64_t)(p + 127) << 23;
        run_range(lo, lo + (1u << 23), threads);
    }
    const unsigned long long binades = g_checked;

    // 2. +-4 ulps of every power of ten in the float range (and of its negative), subnormals included
    std::vector<float> singles;
    for (int k = -45; k <= 38; ++k) {
        char s[16];
        snprintf(s, sizeof s, "1e%d", k);
        const float c = strtof(s, nullptr);
        uint32_t b;
        memcpy(&b, &c, 4);
        for (int d = -4; d <= 4; ++d)
            if ((int64_t)b + d >= 0) {
                singles.push_back(from_bits(b + d));
                singles.push_back(-from_bits(b + d));
            }
    }
    // 3. the specials: zeros, infinities, both NaN signs, subnormals, FLT_MAX, FLT_MIN, the issue's cases
    const float specials[] = {0.0f, -0.0f, INFINITY, -INFINITY, from_bits(0x7fc00000u), from_bits(0xffc00000u),
                              from_bits(0x7f800001u), from_bits(0xff800001u), from_bits(0x7fffffffu), from_bits(0xffffffffu),
                              from_bits(1u), from_bits(0x80000001u), from_bits(0x007fffffu), from_bits(0x00400000u),
                              FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, FLT_EPSILON, 1234565.f, 123456.5f, 999999.5f, 1e-05f,
                              0.0001f, 99999.95f, 0.5f, 1.0f, 100000.0f, 1000000.0f};
    for (float f : specials) singles.push_back(f);
    for (uint32_t b = 0; b < 4096; ++b) singles.push_back(from_bits(b)); // the smallest subnormals
    for (float f : singles) check_float(f);
    g_checked += singles.size();

    // 4. every 7-digit tie: integers in [1e6, 1.6e7) that end in 5, and x.5 in [1e5, 1e6) (all exact floats)
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([=] {
                unsigned long long n = 0;
                for (uint32_t i = 1000005u + 10u * t; i < 16000000u; i += 10u * threads, ++n) {
                    check_float((float)i);
                    check_float(-(float)i);
                }
                for (uint32_t i = 100000u + t; i < 1000000u; i += threads, ++n) check_float((float)i + 0.5f);
                g_checked += n;
            });
        for (auto &th : pool) th.join();
    }

    // 5. random bit patterns
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([=] {
                uint64_t s = 0x5eed0000ull + t;
                unsigned long long n = 0;
                for (unsigned long long i = t; i < randoms; i += threads, ++n) check_float(from_bits((uint32_t)splitmix(s)));
                g_checked += n;
            });
        for (auto &th : pool) th.join();
    }

    // 6. unsigned text: colours, 32-bit indices up to UINT32_MAX, size_t counts
    unsigned long long nu = 0;
    for (uint32_t v = 0; v < 1000000u; ++v, ++nu) check_unsigned(v);
    for (uint64_t p = 1; p != 0 && p <= 10000000000000000000ull; p *= 10) {
        for (int d = -2; d <= 2; ++d, nu += 2) {
            const uint64_t v = p + d;
            check_unsigned((uint32_t)v);
            check_unsigned((size_t)v);
        }
        if (p > UINT64_MAX / 10) break;
    }
    const uint64_t edges[] = {UINT32_MAX, UINT32_MAX - 1ull, UINT32_MAX + 1ull, UINT64_MAX, SIZE_MAX, 4294967296ull * 3 + 7};
    for (uint64_t v : edges) {
        check_unsigned((uint32_t)v);
        check_unsigned((size_t)v);
        nu += 2;
    }
    uint64_t s = 42;
    for (int i = 0; i < 1000000; ++i, nu += 2) {
        const uint64_t v = splitmix(s);
        check_unsigned((uint32_t)v);
        check_unsigned((size_t)(v >> (v & 63)));
    }
    g_checked += nu;

    if (g_bad) {
        fprintf(stderr, "%llu of %llu values differ\n", (unsigned long long)g_bad, (unsigned long long)g_checked);
        return 1;
    }
    printf("ok: %llu values (%llu in whole binades, %llu random patterns) identical to snprintf\n",
           (unsigned long long)g_checked, binades, randoms);
    return 0;
}
