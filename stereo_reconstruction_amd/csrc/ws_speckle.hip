// ws_speckle.hip -- the speckle filter (OpenCV's filterSpeckles; extension, the rules are in include/ws_stereo.h).
// Connected-component labelling of the whole map, then every pixel of a small region set to new_val.  Four kernels, each
// reading what other workgroups wrote only across a kernel boundary or through the value a device-scope atomic returned;
// no workgroup ever waits for another:
//   * ws_speckle_local_kernel: one workgroup per kSpTW x kSpTH tile.  Runs of horizontal joins from a wave ballot (a tile
//     row is one wave), then union-find in LDS over the vertical joins between runs (atomicMin on LDS roots), then each pixel's label = the map index of its tile-local root, and the local size of each local
//     root.  A region with no join across its tile's edge is complete here: its size goes straight into `count`.
//   * ws_speckle_merge_kernel: one lane per pair of pixels across a tile edge.  Joined pairs run a lock-free union on the
//     global parent array of local roots (a pair whose predecessor along the edge joins the same two local regions leaves
//     the union to it): atomicMin(&parent[b], a) links root b under a < b; if it returns another value
//     than b, b was no longer a root and the union goes on from that value.  Every step strictly lowers the larger index,
//     so it ends however stale a find's read was.
//   * ws_speckle_size_kernel: every local root of a region that crosses a tile edge finds its global root (the parents
//     are final after the boundary), points its parent there, and adds its local size into the root's count: one atomic
//     per local region, skipped once the count is already above max_size (counts only grow).
//   * ws_speckle_apply_kernel: one hop to the global root, the region's count, new_val stored into a removed pixel with a
//     plain vector store.  Pixels and regions (the root pixel of a removed region) are counted with wave ballots into
//     kSpeckleSlots spread-out counters per quantity; ws_speckle_count_kernel sums them.
// Every store is a plain vector store or a vector / LDS atomic.
#include "ws_device.h"
#include "ws_kernels.h"

namespace wsamd {

constexpr int kSpTW = 64, kSpTH = 32;             // tile: one wave-wide row, 32 rows
constexpr int kSpTile = kSpTW * kSpTH;
constexpr int kSpThreads = 256;
constexpr int kSpPer = kSpTile / kSpThreads;      // pixels per lane in the local kernel
constexpr int kSpMaxBlocks = 1 << 20;             // grid-stride beyond this (a grid's work-items must fit 32 bits)
constexpr int kSpApplyBlocks = 2048;              // the apply kernel's grid: few counter atomics
static_assert(kSpTW == 64, "a tile row is one wave");
static_assert(kSpeckleSlots == 64, "ws_speckle_count_kernel: one lane per counter slot");

__device__ __forceinline__ bool sp_joins(float a, float b, float nv, float md)
{
    return a != nv && b != nv && fabsf(a - b) <= md; // (NaN joins nothing)
}

// LDS union-find: lab[p] <= p, roots have lab[p] == p
__device__ __forceinline__ int sp_lds_find(int *lab, int p)
{
    int q;
    while ((q = __hip_atomic_load(&lab[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != p) p = q;
    return p;
}

__device__ __forceinline__ void sp_lds_union(int *lab, int a, int b)
{
    for (;;) {
        a = sp_lds_find(lab, a);
        b = sp_lds_find(lab, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&lab[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == b) return;
        b = old; // b had been linked meanwhile: join a with what it was linked to
    }
}

// the global parent array: parent[x] <= x at every local root x
__device__ __forceinline__ int sp_find(int *parent, int x)
{
    int q;
    while ((q = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = q;
    return x;
}

__global__ __launch_bounds__(kSpThreads) void ws_speckle_local_kernel(SpeckleArgs a)
{
    __shared__ float v[kSpTile];
    __shared__ int lab[kSpTile]; // -1: blank
    __shared__ int sz[kSpTile];
    __shared__ int cross[kSpTile];
    const int t = threadIdx.x, lane = t & 63;
    const int ntx = (a.w + kSpTW - 1) / kSpTW, nty = (a.h + kSpTH - 1) / kSpTH;
    const long long ntiles = (long long)ntx * nty;
    const float nv = a.new_val, md = a.max_diff;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx0 = (int)(tile % ntx) * kSpTW, ty0 = (int)(tile / ntx) * kSpTH;
        for (int k = 0; k < kSpPer; ++k) {
            const int p = k * kSpThreads + t, x = tx0 + (p & (kSpTW - 1)), y = ty0 + p / kSpTW;
            const float val = x < a.w && y < a.h ? a.map[(size_t)y * a.stride + x] : nv; // (outside the map: blank)
            v[p] = val;
            sz[p] = 0;
            cross[p] = 0;
        }
        __syncthreads();
        // runs: a wave holds one tile row; a pixel's label starts as the first pixel of its run of horizontal joins (the
        // highest lane at or left of it that does not join its left neighbour), so only vertical joins need a union
        for (int k = 0; k < kSpPer; ++k) {
            const int p = k * kSpThreads + t;
            const float val = v[p];
            const unsigned long long joined = __ballot(lane > 0 && sp_joins(val, v[p - 1], nv, md)); // (bit 0 never set)
            const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
            const int start = 63 - __clzll(~joined & upto);
            lab[p] = val == nv ? -1 : p - lane + start;
        }
        __syncthreads();
        for (int k = 0; k < kSpPer; ++k) {
            const int p = k * kSpThreads + t, lx = p & (kSpTW - 1), ly = p / kSpTW;
            const float val = v[p];
            if (ly == 0 || !sp_joins(val, v[p - kSpTW], nv, md)) continue;
            // the same two runs were joined by the left neighbour already (its union, or the one its left neighbour ran)
            if (lx > 0 && sp_joins(val, v[p - 1], nv, md) && sp_joins(v[p - kSpTW], v[p - kSpTW - 1], nv, md) &&
                sp_joins(v[p - 1], v[p - kSpTW - 1], nv, md))
                continue;
            sp_lds_union(lab, p, p - kSpTW);
        }
        __syncthreads();
        int root[kSpPer];
        for (int k = 0; k < kSpPer; ++k) {
            const int p = k * kSpThreads + t;
            root[k] = v[p] == nv ? -1 : sp_lds_find(lab, p);
        }
        for (int k = 0; k < kSpPer; ++k) {
            // local sizes: the lanes that share the wave's first root add once through one lane (a tile-wide region
            // would otherwise put 64 same-address LDS atomics into every instruction)
            const int r = root[k];
            const unsigned long long valid = __ballot(r >= 0);
            const int leader = valid ? __ffsll((long long)valid) - 1 : 0;
            const int r0 = __shfl(r, leader);
            const unsigned long long same = __ballot(r >= 0 && r == r0);
            if (lane == leader && valid) atomicAdd(&sz[r0], __popcll(same));
            else if (r >= 0 && r != r0) atomicAdd(&sz[r], 1);
            // a join across the tile's edge: the region is not complete in this tile
            if (r >= 0) {
                const int p = k * kSpThreads + t, lx = p & (kSpTW - 1), ly = p / kSpTW, x = tx0 + lx, y = ty0 + ly;
                const float val = v[p];
                const float *row = a.map + (size_t)y * a.stride;
                bool c = false;
                if (lx == 0 && x > 0) c |= sp_joins(val, row[x - 1], nv, md);
                if (lx == kSpTW - 1 && x + 1 < a.w) c |= sp_joins(val, row[x + 1], nv, md);
                if (ly == 0 && y > 0) c |= sp_joins(val, a.map[(size_t)(y - 1) * a.stride + x], nv, md);
                if (ly == kSpTH - 1 && y + 1 < a.h) c |= sp_joins(val, a.map[(size_t)(y + 1) * a.stride + x], nv, md);
                if (c) cross[r] = 1;
            }
        }
        __syncthreads();
        for (int k = 0; k < kSpPer; ++k) {
            const int p = k * kSpThreads + t, x = tx0 + (p & (kSpTW - 1)), y = ty0 + p / kSpTW;
            if (x >= a.w || y >= a.h) continue;
            const int r = root[k];
            const size_t gi = (size_t)y * a.w + x;
            a.label[gi] = r < 0 ? -1 : (int)((size_t)(ty0 + r / kSpTW) * a.w + tx0 + (r & (kSpTW - 1)));
            if (r == p) {
                a.parent[gi] = (int)gi;
                const int n = sz[p];
                a.count[gi] = cross[p] ? 0 : n;
                a.local[gi] = cross[p] ? n : 0;
            }
        }
        __syncthreads(); // (the next tile's loads overwrite the LDS)
    }
}

// pairs: (ntx - 1) * h across the vertical tile edges, then (nty - 1) * w across the horizontal ones
__global__ __launch_bounds__(kSpThreads) void ws_speckle_merge_kernel(SpeckleArgs a, long long n_vertical, long long n_pairs)
{
    const float nv = a.new_val, md = a.max_diff;
    for (long long i = (long long)blockIdx.x * kSpThreads + threadIdx.x; i < n_pairs; i += (long long)gridDim.x * kSpThreads) {
        int x, y, x2, y2;
        if (i < n_vertical) {
            y = (int)(i % a.h);
            x = (int)(i / a.h + 1) * kSpTW - 1;
            x2 = x + 1;
            y2 = y;
        } else {
            const long long j = i - n_vertical;
            x = (int)(j % a.w);
            y = (int)(j / a.w + 1) * kSpTH - 1;
            x2 = x;
            y2 = y + 1;
        }
        int ra = a.label[(size_t)y * a.w + x], rb = a.label[(size_t)y2 * a.w + x2];
        if (ra < 0 || rb < 0 || ra == rb) continue;
        if (!sp_joins(a.map[(size_t)y * a.stride + x], a.map[(size_t)y2 * a.stride + x2], nv, md)) continue;
        // the previous pair along the edge (the row above, or the column to the left) joins the same two local regions:
        // its lane runs this union (or the one before it does), so a long shared edge costs one union, not one per pixel
        const int px = i < n_vertical ? x : x - 1, py = i < n_vertical ? y - 1 : y;
        const int px2 = i < n_vertical ? x2 : x2 - 1, py2 = i < n_vertical ? y2 - 1 : y2;
        if (px >= 0 && py >= 0 && a.label[(size_t)py * a.w + px] == ra && a.label[(size_t)py2 * a.w + px2] == rb &&
            sp_joins(a.map[(size_t)py * a.stride + px], a.map[(size_t)py2 * a.stride + px2], nv, md))
            continue;
        for (;;) {
            ra = sp_find(a.parent, ra);
            rb = sp_find(a.parent, rb);
            if (ra == rb) break;
            if (ra > rb) { const int t = ra; ra = rb; rb = t; }
            const int old = __hip_atomic_fetch_min(&a.parent[rb], ra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == rb) break;
            rb = old; // rb had been linked meanwhile: join ra with what it was linked to
        }
    }
}

__global__ __launch_bounds__(kSpThreads) void ws_speckle_size_kernel(SpeckleArgs a, long long n)
{
    for (long long i = (long long)blockIdx.x * kSpThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSpThreads) {
        if (a.label[i] != (int)i) continue;
        const int loc = a.local[i];
        if (!loc) continue; // (complete in its tile: count holds its size)
        const int r = sp_find(a.parent, (int)i);
        if (r != (int)i) a.parent[i] = r; // (every value on the way leads to r: a concurrent find may read either)
        if (a.count[r] <= a.max_size) __hip_atomic_fetch_add(&a.count[r], loc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kSpThreads) void ws_speckle_apply_kernel(SpeckleArgs a, long long n, unsigned long long *slots)
{
    unsigned long long pixels = 0, regions = 0; // this wave's (the same in every lane)
    for (long long i0 = (long long)blockIdx.x * kSpThreads; i0 < n; i0 += (long long)gridDim.x * kSpThreads) {
        const long long i = i0 + threadIdx.x;
        bool removed = false, root = false;
        if (i < n) {
            const int l = a.label[i];
            if (l >= 0) {
                const int r = a.parent[l];
                removed = a.count[r] <= a.max_size;
                root = removed && r == (int)i;
                if (removed) {
                    const long long y = i / a.w, x = i - y * a.w;
                    a.map[(size_t)y * a.stride + x] = a.new_val;
                }
            }
        }
        pixels += (unsigned long long)__popcll(__ballot(removed));
        regions += (unsigned long long)__popcll(__ballot(root));
    }
    const int slot = (blockIdx.x * (kSpThreads / 64) + (threadIdx.x >> 6)) % kSpeckleSlots;
    if ((threadIdx.x & 63) == 0) {
        if (pixels) atomicAdd(&slots[slot * kSpeckleSlotWords], pixels);
        if (regions) atomicAdd(&slots[(kSpeckleSlots + slot) * kSpeckleSlotWords], regions);
    }
}

// counts[k] = the sum of quantity k's kSpeckleSlots counters: one wave per quantity
__global__ __launch_bounds__(128) void ws_speckle_count_kernel(const unsigned long long *slots, unsigned long long *counts)
{
    unsigned long long v = slots[threadIdx.x * kSpeckleSlotWords];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) counts[threadIdx.x >> 6] = v;
}

hipError_t launch_speckle(const SpeckleArgs &a, unsigned long long *slots, unsigned long long *counts, hipStream_t s)
{
    const long long n = (long long)a.w * a.h;
    const long long ntx = (a.w + kSpTW - 1) / kSpTW, nty = (a.h + kSpTH - 1) / kSpTH;
    const long long n_vertical = (ntx - 1) * a.h, n_pairs = n_vertical + (nty - 1) * a.w;
    auto blocks = [](long long items, long long cap) { return (unsigned)std::max(1LL, std::min((items + kSpThreads - 1) / kSpThreads, cap)); };
    hipLaunchKernelGGL(ws_speckle_local_kernel, dim3((unsigned)std::min(ntx * nty, (long long)kSpMaxBlocks)), dim3(kSpThreads), 0, s, a);
    if (n_pairs) hipLaunchKernelGGL(ws_speckle_merge_kernel, dim3(blocks(n_pairs, kSpMaxBlocks)), dim3(kSpThreads), 0, s, a, n_vertical, n_pairs);
    hipLaunchKernelGGL(ws_speckle_size_kernel, dim3(blocks(n, kSpMaxBlocks)), dim3(kSpThreads), 0, s, a, n);
    hipLaunchKernelGGL(ws_speckle_apply_kernel, dim3(blocks(n, kSpApplyBlocks)), dim3(kSpThreads), 0, s, a, n, slots);
    hipLaunchKernelGGL(ws_speckle_count_kernel, dim3(1), dim3(2 * kSpeckleSlots), 0, s, slots, counts);
    return hipGetLastError();
}

} // namespace wsamd
