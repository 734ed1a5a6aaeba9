// ws_mesh.hip -- WriteMesh (reconstruction.cpp:72-149) with CheckTriangularValidity (:46-69) on the device: the COFF
// text of a w x h vertex grid, byte for byte what ws_write_mesh_off (ws_io.cpp) writes.
//
// An ITEM is one line of the text before the face lines are filtered: items [0, w*h) are the vertex lines, items
// w*h + c are the grid cells c in row-major order, each carrying the 0, 1 or 2 face lines of its triangles
// (i00, i10, i01) and (i10, i11, i01).  Item i's text starts where the text of items [0, i) ends, so three launches
// lay the file out without any workgroup waiting on another (reduce-then-scan, no look-back):
//   1. ws_mesh_count_kernel: every workgroup of kMeshThreads items sums its bytes and faces;
//   2. ws_mesh_scan_kernel (one workgroup): exclusive byte offsets of the workgroups, the face count, the header size;
//   3. ws_mesh_write_kernel: every workgroup formats its items into LDS, packed, and stores the run with dword stores;
//      workgroup 0 also writes the header "COFF\n<w*h> <faces> 0\n".
// Pass 3 formats what pass 1 measured with the same code (ws_text.h): the offsets are exact.
#include "ws_kernels.h"
#include "ws_text.h"

#include <math.h>

namespace wsamd {
namespace {

using namespace text;

constexpr int kMeshThreads = 256;      // items per workgroup in passes 1 and 3
constexpr int kMeshItemBytes = 72;     // >= the longest item: a vertex line (3 * 12 + 4 * 3 + 7 = 55), two face lines (2 * 35)
constexpr int kMeshScanThreads = 1024;

struct MeshGeom {
    const float4 *pos;
    const uchar4 *col;
    uint32_t w, h;
    unsigned long long verts, items; // w * h, w * h + (w - 1) * (h - 1)
    float thr;
};

// CheckTriangularValidity (reconstruction.cpp:46-69) as mesh_triangle_ok (ws_io.cpp) evaluates it: the edge lengths
// are sqrtf(dx*dx + dy*dy + dz*dz), every operation rounded on its own (powf(x, 2) is x*x), and the test keeps its
// negated form so that NaN lengths and a NaN threshold pass as they do on the host.  sqrtf, not __fsqrt_rn: HIP's
// __fsqrt_rn is the bare v_sqrt_f32 (1 ulp); sqrtf is correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt (v_sqrt_f32 and an fma correction step)
__device__ inline float edge_len(float4 p, float4 q)
{
    const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

__device__ inline bool triangle_ok(float4 a, float4 b, float4 c, float thr)
{
    const float minf = -INFINITY;
    if (a.x == minf || b.x == minf || c.x == minf) return false;
    return !(edge_len(a, b) > thr || edge_len(a, c) > thr || edge_len(b, c) > thr);
}

// One item, decoded: its length first (pass 1 and 3), then its text (pass 3).
struct Item {
    int kind = 0;          // 0 = nothing (past the end), 1 = vertex, 2 = valid vertex (coordinates printed), 3 = cell
    G6 g[3];               // the coordinates' %g digits
    uchar4 c;              // colour
    uint32_t i00 = 0, w = 0;
    bool ok0 = false, ok1 = false;
    int faces = 0;

    __device__ void load(const MeshGeom &m, unsigned long long item)
    {
        if (item < m.verts) {
            const float4 p = m.pos[item];
            c = m.col[item];
            kind = p.x == -INFINITY ? 1 : 2;
            if (kind == 2) {
                g[0] = g6_decompose(p.x);
                g[1] = g6_decompose(p.y);
                g[2] = g6_decompose(p.z);
            }
        } else if (item < m.items) {
            kind = 3;
            w = m.w;
            const uint32_t cell = (uint32_t)(item - m.verts), x = cell % (w - 1), y = cell / (w - 1);
            i00 = y * w + x;
            const float4 p00 = m.pos[i00], p01 = m.pos[i00 + 1], p10 = m.pos[i00 + w], p11 = m.pos[i00 + w + 1];
            ok0 = triangle_ok(p00, p10, p01, m.thr);
            ok1 = triangle_ok(p10, p11, p01, m.thr);
            faces = ok0 + ok1;
        }
    }

    __device__ int length() const
    {
        if (kind == 0) return 0;
        if (kind == 3) {
            const int l00 = u_length(i00), l10 = u_length(i00 + w), l01 = u_length(i00 + 1), l11 = u_length(i00 + w + 1);
            return (ok0 ? 5 + l00 + l10 + l01 : 0) + (ok1 ? 5 + l10 + l11 + l01 : 0); // "3 a b c\n"
        }
        const int xyz = kind == 1 ? 6 : g6_length(g[0]) + g6_length(g[1]) + g6_length(g[2]) + 3;
        return xyz + u_length((uint32_t)c.x) + u_length((uint32_t)c.y) + u_length((uint32_t)c.z) + u_length((uint32_t)c.w) + 4;
    }

    __device__ static int face(char *o, uint32_t a, uint32_t b, uint32_t cc)
    {
        int n = 0;
        o[n++] = '3';
        o[n++] = ' ';
        n += u_format(a, o + n);
        o[n++] = ' ';
        n += u_format(b, o + n);
        o[n++] = ' ';
        n += u_format(cc, o + n);
        o[n++] = '\n';
        return n;
    }

    __device__ void write(char *o) const
    {
        if (kind == 0) return;
        int n = 0;
        if (kind == 3) {
            if (ok0) n += face(o + n, i00, i00 + w, i00 + 1);
            if (ok1) face(o + n, i00 + w, i00 + w + 1, i00 + 1);
            return;
        }
        if (kind == 1) {
            for (int k = 0; k < 3; ++k) { o[n++] = '0'; o[n++] = ' '; }
        } else {
            for (int k = 0; k < 3; ++k) { n += g6_write(g[k], o + n); o[n++] = ' '; }
        }
        n += u_format((uint32_t)c.x, o + n);
        o[n++] = ' ';
        n += u_format((uint32_t)c.y, o + n);
        o[n++] = ' ';
        n += u_format((uint32_t)c.z, o + n);
        o[n++] = ' ';
        n += u_format((uint32_t)c.w, o + n);
        o[n++] = '\n';
    }
};

__global__ void __launch_bounds__(kMeshThreads) ws_mesh_count_kernel(MeshGeom m, uint2 *__restrict__ sums)
{
    __shared__ uint32_t red[2][kMeshThreads / 64];
    Item it;
    it.load(m, (unsigned long long)blockIdx.x * kMeshThreads + threadIdx.x);
    uint32_t bytes = (uint32_t)it.length(), faces = (uint32_t)it.faces;
    for (int o = 32; o > 0; o >>= 1) {
        bytes += __shfl_down(bytes, o, 64);
        faces += __shfl_down(faces, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = bytes; red[1][threadIdx.x >> 6] = faces; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 s = make_uint2(0, 0);
        for (int k = 0; k < kMeshThreads / 64; ++k) { s.x += red[0][k]; s.y += red[1][k]; }
        sums[blockIdx.x] = s;
    }
}

// one workgroup: block_off[b] = bytes of workgroups [0, b); meta = {header bytes, file bytes, faces}
__global__ void __launch_bounds__(kMeshScanThreads) ws_mesh_scan_kernel(const uint2 *__restrict__ sums, unsigned long long nb,
                                                                        unsigned long long *__restrict__ block_off,
                                                                        unsigned long long *__restrict__ meta,
                                                                        unsigned long long verts)
{
    __shared__ unsigned long long sc[kMeshScanThreads];
    const int t = threadIdx.x;
    unsigned long long running = 0, faces = 0;
    for (unsigned long long base = 0; base < nb; base += kMeshScanThreads) {
        const unsigned long long i = base + t;
        const uint2 s = i < nb ? sums[i] : make_uint2(0, 0);
        faces += s.y;
        sc[t] = s.x;
        __syncthreads();
        for (int o = 1; o < kMeshScanThreads; o <<= 1) { // inclusive scan (Hillis-Steele)
            const unsigned long long v = t >= o ? sc[t - o] : 0;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        if (i < nb) block_off[i] = running + sc[t] - s.x;
        running += sc[kMeshScanThreads - 1];
        __syncthreads();
    }
    sc[t] = faces;
    __syncthreads();
    for (int o = kMeshScanThreads / 2; o > 0; o >>= 1) {
        if (t < o) sc[t] += sc[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const unsigned long long hdr = 5 + u_length(verts) + 1 + u_length(sc[0]) + 3; // "COFF\n" v " " f " 0\n"
        meta[0] = hdr;
        meta[1] = hdr + running;
        meta[2] = sc[0];
    }
}

__global__ void __launch_bounds__(kMeshThreads) ws_mesh_write_kernel(MeshGeom m, const unsigned long long *__restrict__ block_off,
                                                                     const unsigned long long *__restrict__ meta,
                                                                     char *__restrict__ text)
{
    __shared__ char buf[kMeshThreads * kMeshItemBytes];
    __shared__ uint32_t sc[kMeshThreads];
    const int t = threadIdx.x;
    Item it;
    it.load(m, (unsigned long long)blockIdx.x * kMeshThreads + t);
    const uint32_t len = (uint32_t)it.length();
    sc[t] = len;
    __syncthreads();
    for (int o = 1; o < kMeshThreads; o <<= 1) {
        const uint32_t v = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    const uint32_t total = sc[kMeshThreads - 1];
    it.write(buf + (sc[t] - len));
    __syncthreads();
    // the workgroup's run [g0, g0 + total) of the file: byte stores up to the first 4-byte boundary and after the last,
    // dword stores in between (the neighbours own the bytes around the run)
    const unsigned long long g0 = meta[0] + block_off[blockIdx.x];
    const uint32_t head = (uint32_t)min<unsigned long long>((4 - (g0 & 3)) & 3, total);
    const uint32_t body = (total - head) & ~3u;
    for (uint32_t i = t; i < head; i += kMeshThreads) text[g0 + i] = buf[i];
    for (uint32_t j = t; j < body / 4; j += kMeshThreads) {
        const uint32_t k = head + 4 * j;
        const uint32_t v = (uint32_t)(uint8_t)buf[k] | (uint32_t)(uint8_t)buf[k + 1] << 8 | (uint32_t)(uint8_t)buf[k + 2] << 16 |
                           (uint32_t)(uint8_t)buf[k + 3] << 24;
        *reinterpret_cast<uint32_t *>(text + g0 + k) = v;
    }
    for (uint32_t i = head + body + t; i < total; i += kMeshThreads) text[g0 + i] = buf[i];
    if (blockIdx.x == 0 && t == 0) {
        char *o = text;
        int n = 0;
        o[n++] = 'C'; o[n++] = 'O'; o[n++] = 'F'; o[n++] = 'F'; o[n++] = '\n';
        n += u_format(m.verts, o + n);
        o[n++] = ' ';
        n += u_format(meta[2], o + n);
        o[n++] = ' '; o[n++] = '0'; o[n++] = '\n';
    }
}

MeshGeom mesh_geom(const float *pos, const uint8_t *col, int w, int h, float thr)
{
    MeshGeom m;
    m.pos = reinterpret_cast<const float4 *>(pos);
    m.col = reinterpret_cast<const uchar4 *>(col);
    m.w = (uint32_t)w;
    m.h = (uint32_t)h;
    m.verts = (unsigned long long)w * h;
    m.items = m.verts + (unsigned long long)(w - 1) * (h - 1);
    m.thr = thr;
    return m;
}

} // namespace

size_t mesh_blocks(int w, int h)
{
    const unsigned long long items = (unsigned long long)w * h + (unsigned long long)(w - 1) * (h - 1);
    return (size_t)((items + kMeshThreads - 1) / kMeshThreads);
}

hipError_t launch_mesh_count(const float *pos, const uint8_t *col, int w, int h, float thr, uint32_t *sums,
                             unsigned long long *block_off, unsigned long long *meta, hipStream_t s)
{
    const MeshGeom m = mesh_geom(pos, col, w, h, thr);
    const size_t nb = mesh_blocks(w, h);
    hipLaunchKernelGGL(ws_mesh_count_kernel, dim3((unsigned)nb), dim3(kMeshThreads), 0, s, m, reinterpret_cast<uint2 *>(sums));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, reinterpret_cast<const uint2 *>(sums),
                       (unsigned long long)nb, block_off, meta, m.verts);
    return hipGetLastError();
}

hipError_t launch_mesh_write(const float *pos, const uint8_t *col, int w, int h, float thr, const unsigned long long *block_off,
                             const unsigned long long *meta, char *text, hipStream_t s)
{
    const MeshGeom m = mesh_geom(pos, col, w, h, thr);
    hipLaunchKernelGGL(ws_mesh_write_kernel, dim3((unsigned)mesh_blocks(w, h)), dim3(kMeshThreads), 0, s, m, block_off, meta, text);
    return hipGetLastError();
}

} // namespace wsamd
