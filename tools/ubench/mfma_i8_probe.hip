// mfma_i8_probe.hip -- what ws_march_mfma.h assumes of v_mfma_i32_32x32x32_i8, checked against a host loop with random
// int8 data (asymmetric: a transposed result cannot pass):
//   * byte j of lane half h of the first operand multiplies byte j of lane half h of the second, for the rows
//     (first operand: lane & 31 = row of D, second: lane & 31 = column of D) -- any order of K inside will do;
//   * D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// build: hipcc --offload-arch=gfx950 -O2 -o mfma_i8_probe mfma_i8_probe.hip      exit status 0 = both hold
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// A: 32 rows x 32 bytes (row m of D), B: 32 rows x 32 bytes (column n of D); lane l takes bytes [16 h, 16 h + 16) of row l & 31
__global__ void probe(const int8_t *A, const int8_t *B, int *D)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const i32x4 a = *reinterpret_cast<const i32x4 *>(A + 32 * r + 16 * h);
    const i32x4 b = *reinterpret_cast<const i32x4 *>(B + 32 * r + 16 * h);
    i32x16 c;
    for (int i = 0; i < 16; ++i) c[i] = 1000 * i + lane; // (a known C: the accumulate is checked too)
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
    for (int i = 0; i < 16; ++i) D[16 * lane + i] = c[i];
}

int main()
{
    static int8_t hA[32 * 32], hB[32 * 32];
    static int hD[64 * 16];
    srand(12345);
    for (int i = 0; i < 32 * 32; ++i) {
        hA[i] = (int8_t)(rand() % 256 - 128);
        hB[i] = (int8_t)(rand() % 256 - 128);
    }
    hA[5] = -128; hB[5] = -128; hA[40] = 127; hB[72] = -128; // the int8 limits
    int8_t *dA, *dB;
    int *dD;
    if (hipMalloc(&dA, sizeof hA) != hipSuccess || hipMalloc(&dB, sizeof hB) != hipSuccess || hipMalloc(&dD, sizeof hD) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 2;
    }
    hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice);
    hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dD);
    if (hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("kernel or copy failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    int bad = 0;
    for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 16; ++i) {
            const int col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            int want = 1000 * i + lane;
            for (int k = 0; k < 32; ++k) want += (int)hA[32 * row + k] * (int)hB[32 * col + k];
            if (hD[16 * lane + i] != want && bad++ < 8) printf("lane %d reg %d: got %d want %d\n", lane, i, hD[16 * lane + i], want);
        }
    printf("mfma_i32_32x32x32_i8 operand pairing and C/D map: %s (%d of 1024 wrong)\n", bad ? "MISMATCH" : "ok", bad);
    return bad ? 1 : 0;
}
