// ws_kernels.h -- launch interface between the C-ABI host code (ws_capi.cpp) and the
// gfx950 kernels (ws_march / ws_prepass / ws_border / ws_smooth / ws_consumers / ws_mesh / ws_lr / ws_speckle .hip).  Internal; the public boundary is include/ws_stereo.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wsamd {

// Poison added to a key for an invalid candidate; valid keys stay inside (-2^28, 2^28).
constexpr int32_t kPoison = 1 << 29;
constexpr int32_t kValidKeyBound = 1 << 28;

// The "canonical" search every view is reduced to:
//   outputs live on plane A, candidates d in [d_lo, d_hi] look at plane B column x - d + boff.
// LEFT  (BlockSearch.cpp:24-86):  A = left,  B = right, window bs x bs centred.
// RIGHT (BlockSearch.cpp:88-179): A = right, B = left, both mirrored in x so that the
//   reference's cx = x + d becomes x' - d + (w1 - w2); window (bs-1) x (bs-1).
struct Canon {
    int wa, ha, wb, hb;     // plane sizes (pixels)
    int ww, wh;             // window width / height
    int wx0, wy0;           // window origin relative to the output pixel
    int boff;               // B column = x - d + boff
    int d_lo, d_hi;         // inclusive candidate range (clamped to what complete windows allow)
    int d_hi_clipped;       // ... and what the clipped windows of the right view's border ring allow
    int b_lo, b_hi;         // inclusive range of valid B centre columns
    int ox0, ox1, oy0, oy1; // outputs computed by the marching kernel: [ox0,ox1) x [oy0,oy1)
    int prefer_large;       // ties: 1 -> largest d wins (left), 0 -> smallest d (right)
    int mirror;             // canonical x = wa - 1 - original x
    int fallback_neg;       // no valid candidate: store +x (left) or -x (right), original x
    int ssd;                // 1 = SSD (NORM_L2), 0 = SAD (NORM_L1)
};

// Packed planes: one uint32 per pixel (B | G<<8 | R<<16), zero outside the image.
struct Plane {
    uint32_t *data;
    int pitch; // dwords per row
    int pad;   // plane column = image column + pad
};

struct MarchArgs;
typedef void (*MarchFn)(const MarchArgs); // a marching kernel (ws_march_kernel.h)

// The plan of one marching search: the tiling AND the decision which kernel runs it.  march_plan takes that decision
// once; the launcher launches what the plan names, and everything that reads the packed planes afterwards (pack, border
// ring, refine, smoothFactor passes) takes `centred` from here -- nothing works it out again from the Canon.
struct MarchLaunch {
    int x_per_thread, nd_per_thread; // X, ND template choice
    int nxr, nch;                    // x-runs per tile, d-chunks per tile (and pass)
    int passes;                      // d-group passes (1 unless the disparity range is very wide)
    int threads;                     // workgroup size
    int tiles, strips, strip_rows;
    int halo;                        // packed SAD with the halo exchange (march_pk_halo): tiles advance by (nxr - 1) * X columns
    int tile_cols;                   // output columns per tile
    size_t lds_bytes;
    int max_threads;                 // launch-bounds variant (1024 or 768)
    int mfma;                        // 1: the int8 matrix-core SSD kernel (ws_march_mfma.hip) runs this plan; the fields above
                                     // then describe its tile in the stencil kernel's terms (32 runs of 8 columns, 32 chunks of 8 d)
    MarchFn fn, fn_cost;             // the instantiation that runs; fn_cost: its twin that also writes the winners' costs, or null
    const char *name;                // ... as ws_last_launch_info reports it
    int centred;                     // 1: this SSD window's packed planes hold centred (byte - 128) pixels to keep its sums in 32 bits
                                     // (a matrix-kernel plan keeps the stencil plan's value: the planes do not depend on the kernel)
    int tag_bits;                    // SAD: keys are (cost << tag_bits) | global tie tag (0 for the matrix kernel: it has none)
};

// Fill the plan for this problem on a chip of num_cus CUs (tuning values of 0 = automatic).  Returns false if no
// (window, X, ND) instantiation fits.
bool march_plan(const Canon &c, int num_cus, int tune_nxr, int tune_strip_rows, int tune_threads,
                MarchLaunch *out);
// Plane geometry (pad / pitch) the plan needs.
void march_plane_geometry(const Canon &c, const MarchLaunch &m, Plane *a, Plane *b);

struct GenericArgs;
// pack both planes (for the kernels beside the marching kernel that read planes: border ring, refine, smoothFactor passes)
hipError_t launch_pack(const Canon &c, const MarchLaunch &m, const uint8_t *src_a, int stride_a, Plane dst_a, const uint8_t *src_b,
                       int stride_b, Plane dst_b, hipStream_t s);
// What the hot kernel reads and writes: the caller's CV_8UC3 rows themselves (no planes, no pre-pass) -- img_a carries the
// outputs (left view: the left image), img_b the candidates -- and the map.
struct MarchIo {
    const uint8_t *img_a, *img_b;
    int stride_a, stride_b; // bytes
    float *out;
    int16_t *out16;         // see GenericArgs
    int out_pitch;
    int border;             // also write the zeros of the out_w x out_h map outside the marching interior (left view)
    int out_w, out_h;
    void *keys;             // plane of 8-byte keys (wa x ha, pitch in elements), only touched when m.passes > 1
    int keys_pitch;
    int32_t *cost_out;      // optional plane of the winners' costs (SSD: without sum a^2); needs m.fn_cost
    int cost_pitch;
};
hipError_t launch_march(const Canon &c, const MarchLaunch &m, const MarchIo &io, hipStream_t s);

// Brute-force kernels on the original 8-bit images (original coordinates, literal rules).
struct GenericArgs {
    const uint8_t *L;
    const uint8_t *R;
    int w1, h1, s1, w2, h2, s2;
    int view, ssd, block_size, min_d, max_d, linear_range;
    // pixels inside [skip_x0,skip_x1) x [skip_y0,skip_y1) are left to the marching kernel
    int skip_x0, skip_x1, skip_y0, skip_y1;
    float *out;
    int out_pitch;
    int16_t *out16; // if set, the search kernels store the map as 16-bit integers here (same pitch, in elements) instead of floats to `out`:
                    // the caller (ws_capi.cpp) knows every value is an integer in [-32767, 32767]
    // varBlock (right view): per-pixel block size chosen by ws_varblock_kernel, or null
    const int32_t *bs_plane;
    int bs_pitch;
};
hipError_t launch_generic(const GenericArgs &g, hipStream_t s);
// LinearSearch through LDS (falls back to launch_generic for ranges beyond kLinearMaxRange candidates)
constexpr int kLinearMaxRange = 4096;
hipError_t launch_linear(const GenericArgs &g, hipStream_t s);
// Right-view border ring on the packed (mirrored) planes: sliding sums along runs, lanes over d.
hipError_t launch_ring(const Canon &c, const MarchLaunch &m, Plane a, Plane b, const GenericArgs &skip, float *out, int out_pitch,
                       int32_t *cost_out, int cost_pitch, hipStream_t s);
// Sub-pixel refinement (extension): parabola through the integer cost at d-1, d, d+1.
hipError_t launch_refine(const GenericArgs &g, hipStream_t s);
// the same for the marching interior, on the packed planes (launch_refine then skips g's skip rectangle)
hipError_t launch_refine_planes(const Canon &c, const MarchLaunch &m, Plane a, Plane b, float *out, int out_pitch, hipStream_t s);
// smoothFactor != 1, right view / LinearSearch: g.out must hold the d >= 1 search result
// rows the sel plane must be allocated with (whole LDS chunks are copied)
int smooth_sel_rows(int rows);
// smoothFactor in [0,1], left view: g.out holds the smoothFactor-1 result on entry
// top3: smooth_left_top_bytes(w1, h1, s) of scratch (the row-sum volume at its end only for s outside [0,1])
// gave_up: host-visible word (device pointer) a band of the raster pass sets when it gave up waiting (the map is then invalid)
hipError_t launch_smooth_left(const GenericArgs &g, double s, uint32_t *top3, const Canon *canon, const MarchLaunch *plan, Plane pa,
                              Plane pb, unsigned int *gave_up, hipStream_t st);
size_t smooth_left_top_bytes(int w, int h, double s);
// bytes of the bit-plane scratch launch_smooth wants for a w x h map
size_t smooth_planes_bytes(int w, int h);
// canon / plan / pa / pb: the right view's canonical search, its plan and packed planes when the marching kernel ran
// (g's skip rectangle = its interior) together with the cost plane it and the ring kernel wrote,
// else canon == nullptr
hipError_t launch_smooth(const GenericArgs &g, double s, uint8_t *sel, int sel_pitch, unsigned long long *planes,
                         const Canon *canon, const MarchLaunch *plan, Plane pa, Plane pb, const int32_t *cost, int cost_pitch,
                         hipStream_t st);
// nearest-neighbour perspective warp of a float map; minv maps destination -> source pixels
hipError_t launch_warp(const float *src, int sw, int sh, int sp, float *dst, int dw, int dh, int dp,
                       const double minv[9], hipStream_t s);
// What one launcher of the box filter launched, written by the launcher at the launch from the values it launches with
// (ws_last_outliers_forms; the codes are those of ws_outliers_forms in include/ws_stereo.h).
struct OutlierForms {
    int row_kernel = 0; // 0 = not launched, 1 = 32-bit integer rows, 2 = double rows with the prefix in LDS, 3 = direct O(k) rows
    int row_passes = 0; // trips of the row kernel's loading loop (0 for the direct kernel)
    int row_per = 0;    // pixels per thread of the LDS-prefix row kernel's scan (0 for the others)
    int col_band = 0;   // columns per workgroup of the column kernel; 0 = the direct O(k) column kernel
    int row_window = 0; // 1 = short (k <= w: one reflection at most), 2 = periodic (k > w)
    int col_window = 0; // the same for k and h
};
// removeDisparityOutliers (reconstruction.cpp:5-18); scratch = w*h doubles
hipError_t launch_outliers(float *map, int mp, int w, int h, int k, float thr_front, float thr_back, double *scratch,
                           hipStream_t s, OutlierForms *forms = nullptr);
// the same for 8-bit maps (what the pipeline feeds it: an 8-bit PNG), all sums in 32-bit integers.  A map with any
// value that is not an integer in [0, 255] sets *flag (device word, zero on entry) and *host_word (mapped host word)
// and is left untouched: the caller then runs launch_outliers.  scratch = outliers_u32_scratch_bytes(w, h) bytes.
bool outliers_u32_applies(int w, int h, int k, int num_cus);
size_t outliers_u32_scratch_bytes(int w, int h, int num_cus);
hipError_t launch_outliers_u32(float *map, int mp, int w, int h, int k, float thr_front, float thr_back, uint32_t *scratch,
                               uint32_t *flag, unsigned int *host_word, int num_cus, hipStream_t s, OutlierForms *forms = nullptr);
// convertDisparityToDepth + back-projection (reconstruction.cpp:30-43, :152-196); depth / pos+col may be null
hipError_t launch_depth_vertices(const float *disp, int dp, int w, int h, float focal, float baseline, const float k[9],
                                 const uint8_t *bgr, int bstride, float *depth, int zp, float *pos, uint8_t *col,
                                 int input_is_depth, hipStream_t s);
// WriteMesh (reconstruction.cpp:72-149) on the device (ws_mesh.hip): the COFF text of a w x h vertex grid (pos: w*h
// float4, 16-byte aligned; col: w*h uchar4, 4-byte aligned; w*h <= UINT32_MAX).  launch_mesh_count: sums = 2 words per
// workgroup of mesh_blocks(w, h), block_off = 1 word per workgroup, meta = {header bytes, file bytes, faces} on the
// device.  launch_mesh_write then writes meta[1] bytes of text (the whole file) from the same inputs.
size_t mesh_blocks(int w, int h);
hipError_t launch_mesh_count(const float *pos, const uint8_t *col, int w, int h, float thr, uint32_t *sums,
                             unsigned long long *block_off, unsigned long long *meta, hipStream_t s);
hipError_t launch_mesh_write(const float *pos, const uint8_t *col, int w, int h, float thr, const unsigned long long *block_off,
                             const unsigned long long *meta, char *text, hipStream_t s);
// varBlock (BlockSearch.cpp:125-145, right view): per-pixel window growth + search, one wave per pixel.
// bs_plane: w2 x h2 int32 (pitch bs_pitch), max_block: one device int (max grown block size)
hipError_t launch_varblock(const GenericArgs &g, double thres, int32_t *bs_plane, int bs_pitch, int *max_block,
                           hipStream_t s);
// Left-right consistency check (ws_lr.hip; the rules are in include/ws_stereo.h).  Map 0 is the left map (partner column
// x - rint(v)), map 1 the right map (x + rint(v)); in/out pitches in elements.
enum : uint8_t { kLrEmpty = 0, kLrPassed = 1, kLrFailed = 2 };
struct LrMaps {
    const float *in[2];
    float *out[2];
    int w[2], h[2], in_pitch[2], out_pitch[2];
    uint8_t *state[2]; // one byte per pixel (pitch lr_state_pitch(w)), or null: the fill does not run
};
__host__ __device__ inline int lr_state_pitch(int w) { return (w + 3) & ~3; }
// slots: lr_slot_words() counters, zero on entry (one 64-bit atomic per wave into one of kLrSlots per map); counts: 2
// words, then the failed pixels of map 0 and of map 1
constexpr int kLrSlots = 64, kLrSlotWords = 16; // counters 128 bytes apart
constexpr size_t lr_slot_words() { return 2 * kLrSlots * kLrSlotWords; }
hipError_t launch_lr_check(const LrMaps &m, float max_diff, unsigned long long *slots, unsigned long long *counts, hipStream_t s);
// WS_LR_FILL_BACKGROUND: every failed pixel of the outputs from the nearest passed pixels of its row (states from the check)
hipError_t launch_lr_fill(const LrMaps &m, hipStream_t s);
// Speckle filter (ws_speckle.hip; the rules are in include/ws_stereo.h).  The map is filtered in place.  The four int
// planes hold w*h words each, indexed y*w + x (dense, whatever the map's stride): label = the index of the pixel's
// tile-local root (-1: blank), and at local roots only: parent (union-find over local roots), count (the region's size at
// its global root, or the whole size of a region that never leaves its tile) and local (the local size of a region that
// crosses a tile edge, 0 for one that does not).  slots: speckle_slot_words() counters, zero on entry; counts: 2 words,
// then the pixels set to new_val and the regions removed.
struct SpeckleArgs {
    float *map;
    int w, h, stride;
    float new_val, max_diff;
    int max_size;
    int *label, *parent, *count, *local;
};
constexpr int kSpeckleSlots = 64, kSpeckleSlotWords = 16; // counters 128 bytes apart (as the left-right check's)
constexpr size_t speckle_slot_words() { return 2 * kSpeckleSlots * kSpeckleSlotWords; }
hipError_t launch_speckle(const SpeckleArgs &a, unsigned long long *slots, unsigned long long *counts, hipStream_t s);
} // namespace wsamd
