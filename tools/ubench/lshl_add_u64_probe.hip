// lshl_add_u64_probe.hip -- what one v_lshl_add_u64 costs a wave next to one v_lshl_add_u32: the gate of the packed key
// of ws_march_mfma.h (two keys of an accumulator pair from one 64-bit shift-and-add).
//   * two streams of 24 instructions on independent operands (destinations never read again):
//       v_lshl_add_u64 v[d:d+1], v[a:a+1], 4, v[b:b+1]      and      v_lshl_add_u32 v[d], v[a], 5, v[b];
//   * each bare, and with one v_mfma_i32_32x32x32_i8 per 24 of them (the steady step has about one MFMA per 25 VALU);
//   * at one wave per SIMD (a workgroup of 256 threads) and at two (512 threads, the marching kernel's shape); 96 KB of
//     LDS per workgroup keep a second workgroup off the compute unit.
// Every wave brackets its loop with s_memtime and lane 0 writes the difference out; the table is the median over all
// waves of (ticks per loop trip) / 24, next to the same figure from device events at the printed clock ratio.
// build: hipcc --offload-arch=gfx950 -O3 -o lshl_add_u64_probe lshl_add_u64_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kPerTrip = 24; // VALU instructions per loop trip
constexpr int kLdsBytes = 96 * 1024;
#define WS_U64(D, A, B) "v_lshl_add_u64 %" #D ", %" #A ", 4, %" #B "\n"
#define WS_U32(D, A, B) "v_lshl_add_u32 %" #D ", %" #A ", 5, %" #B "\n"
#define WS_X3(S) S S S

// OP 0: v_lshl_add_u32, 1: v_lshl_add_u64, 2: none (the MFMA and the loop alone); MF: one MFMA per trip
template <int OP, bool MF>
__global__ void __launch_bounds__(512) probe(unsigned long long *ticks, uint32_t *sink, int trips, uint32_t seed)
{
    const uint32_t x = threadIdx.x * 2654435761u + seed;
    uint64_t a[8], b[8], k[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        a[c] = ((uint64_t)(x + c) << 32) | (x * (2 * c + 1));
        b[c] = ((uint64_t)(x ^ c) << 32) | (x + 77 * c);
        k[c] = 0;
    }
    uint32_t a32[8], b32[8], d[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a32[c] = (uint32_t)a[c], b32[c] = (uint32_t)b[c], d[c] = 0;
    i32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = (int)x + i;
    const i32x4 ma = {(int)x, (int)(x >> 3), (int)(x * 3), (int)(x ^ 0x55u)};
    const i32x4 mb = {(int)(x + 1), (int)(x >> 5), (int)(x * 7), (int)(x ^ 0xaau)};

    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < trips; ++it) {
        if (MF) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ma, mb, acc, 0, 0, 0);
        // one asm statement per trip: between two of them the compiler pads with s_nop
        if (OP == 1)
            asm volatile(WS_X3(WS_U64(0, 8, 16) WS_U64(1, 9, 17) WS_U64(2, 10, 18) WS_U64(3, 11, 19) WS_U64(4, 12, 20) WS_U64(5, 13, 21) WS_U64(6, 14, 22) WS_U64(7, 15, 23))
                         : "=&v"(k[0]), "=&v"(k[1]), "=&v"(k[2]), "=&v"(k[3]), "=&v"(k[4]), "=&v"(k[5]), "=&v"(k[6]), "=&v"(k[7])
                         : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]),
                           "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7]));
        if (OP == 0)
            asm volatile(WS_X3(WS_U32(0, 8, 16) WS_U32(1, 9, 17) WS_U32(2, 10, 18) WS_U32(3, 11, 19) WS_U32(4, 12, 20) WS_U32(5, 13, 21) WS_U32(6, 14, 22) WS_U32(7, 15, 23))
                         : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7])
                         : "v"(a32[0]), "v"(a32[1]), "v"(a32[2]), "v"(a32[3]), "v"(a32[4]), "v"(a32[5]), "v"(a32[6]), "v"(a32[7]), "v"(b32[0]), "v"(b32[1]),
                           "v"(b32[2]), "v"(b32[3]), "v"(b32[4]), "v"(b32[5]), "v"(b32[6]), "v"(b32[7]));
        if (OP == 2) asm volatile("" ::: "memory");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();

    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) r ^= (uint32_t)k[c] ^ (uint32_t)(k[c] >> 32) ^ d[c];
#pragma unroll
    for (int i = 0; i < 16; ++i) r ^= (uint32_t)acc[i];
    sink[blockIdx.x * blockDim.x + threadIdx.x] = r;
    if ((threadIdx.x & 63) == 0) ticks[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = t1 - t0;
}

static unsigned long long *g_ticks;
static uint32_t *g_sink;
constexpr int kBlocks = 64, kTrips = 200000;

template <int OP, bool MF>
static void run(const char *name, int waves_per_simd)
{
    const int threads = 256 * waves_per_simd, nwaves = kBlocks * threads / 64;
    auto launch = [&](int trips) { hipLaunchKernelGGL((probe<OP, MF>), dim3(kBlocks), dim3(threads), kLdsBytes, 0, g_ticks, g_sink, trips, 1u); };
    hipEvent_t e0, e1;
    hipEventCreate(&e0), hipEventCreate(&e1);
    launch(kTrips); // (warm-up: the code object, the clocks)
    hipDeviceSynchronize();
    hipEventRecord(e0);
    launch(kTrips);
    hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) {
        printf("%s: launch failed: %s\n", name, hipGetErrorString(hipGetLastError()));
        exit(2);
    }
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> t(nwaves);
    hipMemcpy(t.data(), g_ticks, sizeof(unsigned long long) * nwaves, hipMemcpyDeviceToHost);
    std::sort(t.begin(), t.end());
    const double med = (double)t[nwaves / 2] / kTrips, lo = (double)t[0] / kTrips, hi = (double)t[nwaves - 1] / kTrips;
    const int per = OP == 2 ? 1 : kPerTrip;
    printf("%-16s %-5s waves/SIMD=%d : ticks/trip median %8.2f (min %8.2f max %8.2f) -> %6.3f ticks per %s | kernel %7.3f ms, %7.1f ticks/us\n",
           name, MF ? "+mfma" : "bare", waves_per_simd, med, lo, hi, med / per, OP == 2 ? "trip" : "instruction", ms,
           (double)t[nwaves / 2] / (ms * 1e3));
    hipEventDestroy(e0), hipEventDestroy(e1);
}

int main()
{
    if (hipMalloc(&g_ticks, sizeof(unsigned long long) * kBlocks * 8) != hipSuccess || hipMalloc(&g_sink, 4 * kBlocks * 512) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 2;
    }
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    hipFuncSetAttribute(reinterpret_cast<const void *>(probe<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    for (int rep = 0; rep < 2; ++rep)
        for (int w : {1, 2}) {
            run<0, false>("v_lshl_add_u32", w);
            run<1, false>("v_lshl_add_u64", w);
            run<2, true>("(mfma alone)", w);
            run<0, true>("v_lshl_add_u32", w);
            run<1, true>("v_lshl_add_u64", w);
        }
    return 0;
}
