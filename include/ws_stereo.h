/*
 * ws_stereo.h -- C-ABI of the MI355X-native WindowSearch (dense block matching).
 *
 * This is the drop-in boundary for the reference's src/WindowSearch stage: plain
 * pointers and sizes, no OpenCV / torch / C++ types.  Every entry point names
 * the reference interface it replaces (paths relative to the reference root).
 * The C++ facade with the reference's class names lives in
 * stereo_reconstruction_amd/host/window_search.hpp; the binding a maintainer of
 * the reference would add is shown in INTEGRATION.md.
 *
 * All compute runs in hand-written HIP kernels for gfx950.  There is no CPU
 * fallback: without a usable HIP device ws_create() fails with WS_ERR_HIP.
 *
 * Images: 8-bit, 3 channels interleaved in cv::imread order (BGR), row-major,
 * `stride` bytes per row (CV_8UC3, BlockSearch.cpp:41, :105).  Left and right
 * may differ in size (BlockSearch.cpp:25-30).  Disparity maps: row-major,
 * integer-valued unless sub-pixel refinement is on.
 */
#ifndef WS_STEREO_H
#define WS_STEREO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WS_VERSION 100 /* 0.1.0 */

/* status codes (the reference has none: it throws cv::Exception / loops forever) */
enum {
    WS_OK = 0,
    WS_ERR_ARG = -1,         /* null pointer, bad size / stride / enum */
    WS_ERR_GEOMETRY = -2,    /* the reference would throw cv::Exception: even blockSize in the
                                left view (BlockSearch.cpp:46-49), left ROI outside the image in
                                the right view (BlockSearch.cpp:151-154) */
    WS_ERR_UNSUPPORTED = -3, /* legal for the reference, not implemented on the device yet */
    WS_ERR_HIP = -4,         /* HIP runtime error (see ws_last_error) */
    WS_ERR_IO = -5,          /* file could not be read / written / parsed */
    WS_ERR_NOMEM = -6
};

/* which reference method the call stands for */
enum {
    WS_VIEW_LEFT = 0,   /* BlockSearch::computeDisparityMapLeft   (BlockSearch.cpp:24-86)  */
    WS_VIEW_RIGHT = 1,  /* BlockSearch::computeDisparityMapRight  (BlockSearch.cpp:88-179) */
    WS_VIEW_LINEAR = 2  /* LinearSearch::computeDisparityMap      (LinearSearch.cpp:10-59) */
};

enum {
    WS_COST_SSD = 0, /* the reference's cost: cv::norm(absdiff, NORM_L2) (BlockSearch.cpp:64-66) */
    WS_COST_SAD = 1, /* extension: NORM_L1 in the same loops (BASELINE.json configs 1 and 3) */
    /* extension: the Hamming distance of census-transform descriptors ("census-transform matching cost" below) */
    WS_COST_CENSUS_5X5 = 2, /* 24-bit descriptors: neighbourhood rx = 2, ry = 2 */
    WS_COST_CENSUS_9X7 = 3  /* 62-bit descriptors: neighbourhood rx = 4, ry = 3 (9 wide, 7 high) */
};

enum { WS_OUT_F32 = 0, WS_OUT_F64 = 1 }; /* F64 = the reference's CV_64F maps (BlockSearch.cpp:33) */

typedef struct {
    const uint8_t *data; /* host pointer for *_host calls, device pointer for *_device calls */
    int width;
    int height;
    int stride;          /* bytes per row, >= 3 * width */
} ws_image;

/*
 * The constructor + call arguments of the reference, in one struct.
 *   BlockSearch(L, R, blockSize, minDisparity, maxDisparity)        BlockSearch.h:11-15
 *   computeDisparityMapLeft(smoothFactor)                            BlockSearch.h:28
 *   computeDisparityMapRight(smoothFactor, varBlock, thres)          BlockSearch.h:37
 *   LinearSearch(L, R).computeDisparityMap(smoothFactor)             LinearSearch.h:13-19
 * Use ws_params_default() and then set what differs.
 */
typedef struct {
    int view;             /* WS_VIEW_* */
    int cost;             /* WS_COST_* (LINEAR ignores it: always the Euclidean pixel distance) */
    int block_size;       /* blockSize (LINEAR ignores it) */
    int min_disparity;    /* minDisparity: read by the right view only (BlockSearch.cpp:147) */
    int max_disparity;    /* maxDisparity: left tries d = maxD..1, right d = minD..maxD-1 */
    double smooth_factor; /* smoothFactor, any value but NaN (!= 1 in the left view is a true raster-order
                             dependency, SURVEY.md 8f-1: a serial pass of a few ms) */
    int var_block;        /* varBlock (right view): grow the window (block size + 4) while its centred norm < thres;
                             growth stops when the clipped window no longer changes (the reference would loop
                             forever there), and the max block counts that last + 4.  A grown window is not bound
                             by block_size's limit of 63: it can span the whole image (costs summed in 64 bits) */
    double thres;         /* thres for varBlock, default 19.0 (BlockSearch.h:37) */
    int subpixel;         /* extension: parabolic refinement on the aggregated integer cost */
    int linear_range;     /* LinearSearch's hard-coded 200 candidates (LinearSearch.cpp:32) */
} ws_params;

typedef struct ws_context ws_context; /* one per device; not to be shared between threads */

/* ---- life cycle ------------------------------------------------------------------- */
int ws_version(void);
void ws_params_default(ws_params *p);
/* Open HIP device `device`.  Owns a stream, scratch planes and staging buffers. */
int ws_create(int device, ws_context **out);
void ws_destroy(ws_context *ctx);
/* Text of the last error on this context (or of the last failed ws_create if ctx == NULL). */
const char *ws_last_error(const ws_context *ctx);
int ws_device_count(void);

/*
 * The argument checks of the search calls without a device: the status a search with these
 * arguments would return before launching anything (WS_OK, WS_ERR_ARG, WS_ERR_GEOMETRY for
 * what makes the reference throw, WS_ERR_UNSUPPORTED).  Message via ws_last_error(NULL).
 */
int ws_validate(const ws_params *p, const ws_image *left, const ws_image *right);

/* How a search would be tiled on a device with num_cus compute units (0 = 256); host logic only.  Everything in the
 * plan is for that chip: the thread shape (x_per_thread, d_per_thread) as well as the tiles and strips. */
typedef struct {
    int marching;                   /* 1: the marching kernel owns the interior; 0: brute force only */
    int x_per_thread, d_per_thread; /* columns x disparities whose window sums one thread keeps */
    int x_runs, d_chunks;           /* per workgroup: tile = x_runs*x_per_thread columns, all d */
    int threads, tiles, strips, strip_rows, lds_bytes;
    int interior_x0, interior_x1, interior_y0, interior_y1; /* outputs the marching kernel writes */
    int passes;                     /* d-group passes (disparity ranges wider than one tile holds) */
    int tile_cols;                  /* columns a tile hands out: x_runs*x_per_thread, one run less for the halo-exchange SAD kernels */
    int kernel_kind;                /* 0: the stencil marching kernel; 1: the int8 matrix-core SSD kernel (a wave owns 32 columns:
                                       x_runs*x_per_thread is still the tile's width, d_chunks*d_per_thread the candidates a tile holds);
                                       2: the census match kernel (marching 0: it writes the whole map; threads, tiles, strips,
                                       strip_rows, tile_cols, lds_bytes are its own, d_chunks the 64-lane chunks of the range) */
} ws_plan_info;
int ws_plan(const ws_params *p, const ws_image *left, const ws_image *right, int num_cus,
            ws_plan_info *out);

/* ---- the hot path ----------------------------------------------------------------- */
/*
 * Synchronous call on host buffers; replaces
 *   BlockSearch(L,R,bs,minD,maxD).computeDisparityMapLeft/Right(...)   BlockSearch.cpp:24-179
 *   LinearSearch(L,R).computeDisparityMap(s)                           LinearSearch.cpp:10-59
 * as called from ImageRectifier::computeDisparityMapLeft/Right (rectification.cpp:66-88)
 * and rectification_main.cpp:194-195.
 * out: h1 x w1 (LEFT) or h2 x w2 (RIGHT, LINEAR) elements of out_dtype, out_stride in
 * elements.  Copies in, runs, copies out, returns when the map is complete.  Pageable buffers cross
 * through pinned staging memory of the library's -- every entry point taking host buffers does that, and none
 * registers caller memory with the HIP runtime; a buffer the caller has pinned itself is used as it is
 * (INTEGRATION.md section 2).  An integer-valued map crosses PCIe as 16-bit integers and is widened to out_dtype
 * on the host (ws_last_wire_format).
 */
int ws_search_host(ws_context *ctx, const ws_params *p, const ws_image *left,
                   const ws_image *right, void *out, int out_stride, int out_dtype);

/*
 * The same on device-resident buffers (images already in HBM, float32 map written to HBM),
 * enqueued on `stream` (a hipStream_t; NULL = the context's own stream).  Returns after
 * enqueueing; order / wait on the stream as usual.  This is what bench.py times.
 */
int ws_search_device(ws_context *ctx, const ws_params *p, const ws_image *left_dev,
                     const ws_image *right_dev, float *out_dev, int out_stride, void *stream);

/*
 * Batched host form for many independent pairs (BASELINE.json config 4): two pairs are kept in
 * flight -- while one is searched, the next one's images go up and the previous one's map comes
 * down on a second stream.  The images and `out` must stay valid and untouched until ws_wait(),
 * which blocks until every enqueued pair's map has landed in its `out`.
 */
int ws_enqueue_host(ws_context *ctx, const ws_params *p, const ws_image *left,
                    const ws_image *right, void *out, int out_stride, int out_dtype);
int ws_wait(ws_context *ctx);

/*
 * The back-projection the caller of the hot path applies to its result:
 *   cv::warpPerspective(disparityMap_rect, disparityMapLeft, H_.inv(), size, INTER_NEAREST)
 *   (rectification.cpp:70-75, :82-87).  `m` is the 3x3 matrix handed to warpPerspective (row-major,
 *   i.e. H_.inv()); like OpenCV the call inverts it and gathers dst(x,y) = src(round(M^-1 (x,y,1))),
 *   0 outside.  For already rectified pairs m is the identity and this is a copy.
 */
int ws_warp_nearest_host(ws_context *ctx, const double *src, int src_w, int src_h, int src_stride,
                         const double m[9], double *dst, int dst_w, int dst_h, int dst_stride);
int ws_warp_nearest_device(ws_context *ctx, const float *src_dev, int src_w, int src_h, int src_stride,
                           const double m[9], float *dst_dev, int dst_w, int dst_h, int dst_stride,
                           void *stream);

/* ---- rectification of an unrectified pair: the first half of ImageRectifier ------------------ */
/*
 * The size of a rectified image (rectification.cpp:436-483): the four corners (0,0), (w,0), (w,h), (0,h)
 * go through H (perspectiveTransform), then cols = (int)(max_x - min_x), rows = (int)(max_y - min_y),
 * truncated.  The rectified image is NOT translated by min_x / min_y: the reference warps with H as it is,
 * so whatever maps left of column 0 or above row 0 is cut off -- a quirk of the reference, kept.
 * WS_ERR_GEOMETRY if a corner has |w| <= FLT_EPSILON (perspectiveTransform would place it at (0,0)) or the
 * size is < 1 or > 32767.  Host only: no context, no device.
 */
int ws_rectified_size(const double H[9], int width, int height, int *out_w, int *out_h);
/*
 * cv::warpPerspective(src, dst, H, Size(dst_w, dst_h)) of a CV_8UC3 image: INTER_LINEAR, BORDER_CONSTANT 0
 * (rectification.cpp:486-493).  H is the matrix handed to warpPerspective (row-major; the call inverts it,
 * WS_ERR_ARG if singular).  Restates OpenCV 4.x's fixed-point bilinear path (<= 4.10 on x86); later OpenCV
 * releases may differ by one grey level.  Device pointers; dst_stride >= 3 * dst_w bytes.  Only enqueues,
 * on `stream` (NULL = the context's own), like ws_search_device.
 */
int ws_rectify_device(ws_context *ctx, const ws_image *src_dev, const double H[9], uint8_t *dst_dev,
                      int dst_w, int dst_h, int dst_stride, void *stream);
/*
 * ImageRectifier::rectifyImagesAndKeyPoints (image part, rectification.cpp:432-493) followed by
 * computeDisparityMapLeft / computeDisparityMapRight (rectification.cpp:66-88), in one synchronous call:
 * both original images go up, are rectified on the device (left with H = H_, right with Hp = Hp_, sizes from
 * ws_rectified_size), searched as ws_search_host searches, and the rectified map is warped back with
 * H_.inv() (INTER_NEAREST; the reference uses H_ for both views) to the original size of the left image (LEFT)
 * or of the right image (RIGHT).  out: that many elements of out_dtype, out_stride in elements.
 * rect_left / rect_right may be NULL; if given they receive the rectified images (getRectifiedLeft/Right,
 * rectification.cpp:499-505), ws_rectified_size big, strides in bytes.  WS_VIEW_LINEAR is WS_ERR_ARG
 * (ImageRectifier has no linear method); the search's checks apply to the rectified sizes.
 */
int ws_search_unrectified_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                               const double H[9], const double Hp[9], void *out, int out_stride, int out_dtype,
                               uint8_t *rect_left, int rect_left_stride, uint8_t *rect_right, int rect_right_stride);

/* ---- left-right consistency check and occlusion fill (extension) ----------------------------- */
/*
 * Flags the pixels whose disparity the other view does not confirm -- OpenCV's disp12MaxDiff cross-check -- on two
 * float32 maps:
 *   A_L, w_L x h_L: left-view convention, pixel x matches right column x - d  (BlockSearch.cpp:82);
 *   A_R, w_R x h_R: right-view convention, pixel x matches left column x + d  (BlockSearch.cpp:174).
 * For each pixel (y, x) of one map with value v, B is the other map and s = -1 for the left map, +1 for the right map.
 *   1. Empty: v == 0 (-0.0 included) means no disparity.  The output is 0; the pixel is not counted and is never a fill
 *      source.
 *   2. Fail: the pixel fails if v is not finite, or y >= h_B, or the partner column p = x + s * rint(v) lies outside
 *      [0, w_B).  rint rounds half to even (rintf, np.rint); p is computed without integer overflow.
 *   3. Otherwise the pixel passes iff fabsf(v - B(y, p)) <= max_diff, in float32: a NaN partner fails, a partner of 0
 *      fails unless |v| <= max_diff.
 *   4. A pixel that passes keeps v.  A failed pixel becomes 0 (WS_LR_FILL_NONE), or (WS_LR_FILL_BACKGROUND) takes the
 *      nearest pixel that passed on the same output row to its left and the nearest to its right: both present, fminf
 *      of their values (the farther surface); one present, its value; neither, 0.  Only pixels that passed are fill
 *      sources: filled pixels never feed other pixels.
 *   5. The count of a map is the number of its pixels that failed (filled pixels included).
 * max_diff >= 0 (+inf allowed); NaN or negative is WS_ERR_ARG.  An output that overlaps an input or the other output is
 * WS_ERR_ARG.  The rules need no search: they apply to any two maps (sub-pixel maps, maps read from PFM).  A checked map
 * feeds ws_convert_disparity_to_depth as it is: 0 becomes -inf and the mesh drops that vertex (reconstruction.cpp:30-43).
 */
enum { WS_LR_FILL_NONE = 0, WS_LR_FILL_BACKGROUND = 1 };
typedef struct {
    float max_diff; /* the largest |v - partner| that passes (disp12MaxDiff) */
    int fill;       /* WS_LR_FILL_* */
} ws_lr_params;

/* The check alone, on maps in device memory (strides in elements).  Only enqueues, on `stream` (NULL = the context's own). */
int ws_lr_check_device(ws_context *ctx, const float *left_dev, int lw, int lh, int lstride,
                       const float *right_dev, int rw, int rh, int rstride, const ws_lr_params *lr,
                       float *out_left_dev, int out_lstride, float *out_right_dev, int out_rstride, void *stream);
/*
 * Both block-search views of one pair, then the check, on host buffers; synchronous.  p->view is ignored: the call runs p
 * as WS_VIEW_LEFT and then as WS_VIEW_RIGHT, every other field as given, each map bit-identical to ws_search_host's for
 * that view.  Each view's parameters are checked as ws_search_host checks them; the first refusal is returned, left
 * first.  The images go up once; both checked maps come down as out_dtype (F64: the float32 map widened).
 * out_left: h_L x w_L, out_right: h_R x w_R elements, strides in elements.
 */
int ws_search_lr_host(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right,
                      const ws_lr_params *lr, void *out_left, int out_lstride, void *out_right, int out_rstride,
                      int out_dtype);
/* The same on device images and float32 device maps.  Only enqueues; ws_device_status reports the left view's raster pass. */
int ws_search_lr_device(ws_context *ctx, const ws_params *p, const ws_image *left_dev, const ws_image *right_dev,
                        const ws_lr_params *lr, float *out_left_dev, int out_lstride, float *out_right_dev,
                        int out_rstride, void *stream);
/* Pixels that failed in the last check of this context, {left, right}; waits for that check's stream. */
int ws_last_lr_counts(ws_context *ctx, unsigned long long counts[2]);

/* ---- speckle filter (extension) ----------------------------------------------------------- */
/*
 * OpenCV's filterSpeckles (calib3d/src/stereosgbm.cpp, filterSpecklesImpl) on a float32 map A, w x h, `stride` floats
 * per row, in place:
 *   1. A pixel is blank if A(y, x) == new_val (float ==: -0.0 is blank when new_val is 0).  Blank pixels belong to no
 *      region and are left untouched, bits included.
 *   2. Two 4-neighbours join if neither is blank and fabsf(a - b) <= max_diff, in float32: a NaN pixel joins nothing,
 *      and +inf joins nothing unless max_diff is +inf (inf - finite then passes; inf - inf is NaN and never does).
 *   3. A region is a connected component of the graph of those joins.
 *   4. Every pixel of a region of count <= max_speckle_size pixels becomes exactly new_val; every other pixel keeps its
 *      bits.  max_speckle_size == 0 changes nothing.
 *   5. Counts: the pixels set to new_val, and the regions removed.
 *   6. WS_ERR_ARG: new_val NaN; max_diff NaN or negative (+inf allowed); max_speckle_size < 0; a null pointer; w or h < 1;
 *      stride < w; w * h >= 2^31.
 * The rules do not depend on scan order.  On a map whose values, new_val and max_diff are integers in int16 range the
 * result is OpenCV's CV_16SC1 result.  A filtered map with new_val 0 feeds ws_convert_disparity_to_depth as it is.
 */
typedef struct {
    float new_val;        /* the value of blank pixels, and what removed pixels become */
    int max_speckle_size; /* regions of at most this many pixels are removed */
    float max_diff;       /* the largest |a - b| between 4-neighbours of one region */
} ws_speckle_params;

/* In place on a float32 map in device memory.  Only enqueues, on `stream` (NULL = the context's own). */
int ws_filter_speckles_device(ws_context *ctx, float *map_dev, int w, int h, int stride, const ws_speckle_params *sp,
                              void *stream);
/* In place on a float32 map in host memory; synchronous. */
int ws_filter_speckles_host(ws_context *ctx, float *map, int w, int h, int stride, const ws_speckle_params *sp);
/* {pixels set to new_val, regions removed} by the last filter of this context; waits for that filter's stream. */
int ws_last_speckle_counts(ws_context *ctx, unsigned long long counts[2]);

/* ---- semi-global matching (extension) ---------------------------------------------------- */
/*
 * Hirschmueller's cost aggregation along image paths over the block search's exact window costs.  p: view LEFT or
 * RIGHT, cost (SSD, SAD or a census cost), block_size, the disparity range and subpixel, as for ws_search_*; smooth_factor must be 1.  For each pixel
 * p of the output map the block search (smoothFactor 1, no varBlock) defines
 *   * K(p): its candidate disparities, a contiguous interval or empty;
 *   * C(p, d) for d in K(p): the exact integer window cost (SSD: the sum of squares before the square root; right view:
 *     the clipped window's sum before the area division).
 *   1. Node: p lies inside the searched region (left view: rows [half, min(h1,h2) - half), columns [half, w1 - half);
 *      right view: rows < min(h1,h2)), is not black (the view's own black test) and K(p) is not empty.
 *   2. Path cost, for each direction r with predecessor q = p - r.  If q is outside the image or not a node,
 *      Lr(p,d) = C(p,d): paths restart after black pixels, outside the region and at pixels without candidates.  Else,
 *      with m(q) = min over k in K(q) of Lr(q,k):
 *        Lr(p,d) = C(p,d) + min(Lr(q,d), Lr(q,d-1) + P1, Lr(q,d+1) + P1, m(q) + P2) - m(q),
 *      leaving out a term whose disparity is not in K(q); the last term is always there.
 *      paths 4: r = (1,0) (-1,0) (0,1) (0,-1), i.e. predecessors (x-1,y) (x+1,y) (x,y-1) (x,y+1); 8: also the diagonals.
 *   3. S(p,d) = the sum of Lr(p,d) over the paths.  A node's value is the argmin of S over K(p), ties as the view breaks
 *      them: left view the largest d, right view the smallest d.
 *   4. Non-nodes get what the block search stores: not black, no candidate: x (left view) or -x (right view); black or
 *      outside the region: 0.
 *   5. subpixel = 1: num = S(d-1) - S(d+1), den = S(d-1) - 2 S(d) + S(d+1), exact; refined only if d-1 and d+1 are in
 *      K(p) and den > 0, to (float)d + (float)(num / (2.0 * den)).
 *   6. The arithmetic is exact (C < 2^30 for block_size <= 63, Lr <= C + P2 < 2^32, S < 2^35): the storage widths are
 *      picked from a bound on the host, and the map equals the exact one.
 * Identity: with P1 = P2 = 0, S = paths * C for any paths, and the map equals ws_search_* with smoothFactor 1 bit for bit,
 * the sub-pixel map included.
 * Refusals: every refusal of ws_validate; WS_ERR_UNSUPPORTED for WS_VIEW_LINEAR, smooth_factor != 1, var_block in the
 * right view, more than 2048 disparities left after the geometry's clip (left view min(maxD, w1 - 1 - 2 half), right view
 * min(maxD, w1) - minD), a map of 2^31 pixels or more; WS_ERR_ARG for a null sgm, paths not 4 or 8, p1 < 0, p2 < p1.
 * The scratch (ws_sgm_scratch_bytes) belongs to the context and grows on demand; a failed allocation is WS_ERR_NOMEM and
 * leaves the context usable.  A map feeds ws_lr_check_device, ws_filter_speckles_device and the consumers as it is.
 */
typedef struct {
    int paths; /* 4: predecessors (x-1,y) (x+1,y) (x,y-1) (x,y+1); 8: also the four diagonal ones */
    int p1;    /* penalty for a disparity change of 1 between path neighbours, in cost units, >= 0 */
    int p2;    /* penalty for a larger change, >= p1 */
} ws_sgm_params;

/* The argument checks of the SGM calls without a device (message via ws_last_error(NULL)). */
int ws_validate_sgm(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right);
/* Host only: the device memory an SGM call with these arguments would hold. */
int ws_sgm_scratch_bytes(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right,
                         unsigned long long *bytes);
/* On device images into a float32 device map (out_stride floats per row).  Only enqueues, on `stream` (NULL = the
 * context's own), like ws_search_device. */
int ws_search_sgm_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *left_dev,
                         const ws_image *right_dev, float *out_dev, int out_stride, void *stream);
/* On host buffers, synchronous, as ws_search_host (the same staging path); F64 is the float32 map widened. */
int ws_search_sgm_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_image *left,
                       const ws_image *right, void *out, int out_stride, int out_dtype);

/* ---- uniqueness ratio and confidence (extension) --------------------------------------------- */
/*
 * OpenCV's uniquenessRatio for the block search and for SGM: a pixel whose best cost is not clearly better than its best
 * rival is dropped, and the margin itself is available as a confidence plane.  p, the views, K(p), C(p, j), nodes and
 * the fallbacks are those of the SGM section (j = the index of a disparity in the view's range).  S(p, j) depends on
 * `sgm`: non-null, it is that section's sum over the paths; NULL, S = C: the block search at smoothFactor 1 (no path
 * kernel runs and no sum plane is allocated).
 *   1. Winner: jb = argmin of S over K(p) with the view's tie rule (unchanged), Smin = S(p, jb).
 *   2. Rivals: the j in K(p) with |j - jb| >= 2; m2 = the minimum of S over them.  A node without rivals is uncontested:
 *      K(p) is an interval, so these are the nodes with at most 2 candidates and those with 3 whose winner is the
 *      middle one.
 *   3. Fail test: a contested node fails iff m2 * (100 - ratio) < Smin * 100, in exact integers.  This is StereoSGBM's
 *      test, strict `<` included: an exact tie with Smin == 0 (then m2 == 0 too) passes at every ratio.  ratio == 0 fails
 *      nothing; ratio == 100 fails every contested node with Smin > 0.
 *   4. Map: a failed node stores 0.0f ("no disparity", as after the left-right check); a passing node stores exactly what
 *      ws_search_sgm_* stores (sgm == NULL: what ws_search_* stores), the sub-pixel value included; non-nodes are
 *      unchanged (x / -x / 0).
 *   5. Confidence, an optional float32 plane that does not depend on ratio: a contested node with m2 > 0 stores
 *      (float)((double)(m2 - Smin) / (double)m2); a contested node with m2 == 0 stores 0.0f; an uncontested node 1.0f;
 *      a non-node 0.0f.
 *   6. Counts: {failed nodes, nodes} of the last call.
 *   7. Identities: (a) with ratio == 0 the map is ws_search_sgm_*'s (sgm == NULL: ws_search_*'s) bit for bit; (b)
 *      sgm == NULL and sgm = {paths, 0, 0} give the same map and the same confidence (S = paths * C scales both sides of
 *      rule 3 and cancels in rule 5); (c) the fail set grows with ratio.
 *   8. Refusals, without a device: everything ws_validate_sgm refuses (sgm == NULL: the same list without the checks of
 *      sgm itself); WS_ERR_ARG for a null ws_unique_params, ratio outside 0 .. 100, conf_stride < width for a given
 *      confidence plane, or a confidence plane that overlaps the map.
 * The scratch is the SGM calls' own (sgm == NULL: the intervals and C only), so a uniqueness call and an SGM call on two
 * streams order themselves as two SGM calls do.  A map feeds ws_lr_check_device, ws_filter_speckles_device and the
 * consumers as it is (ws_convert_disparity_to_depth: 0 -> -inf, the mesh leaves the vertex out).
 */
typedef struct {
    int ratio; /* 0 .. 100, OpenCV's uniquenessRatio: the margin in percent by which the best cost must win */
} ws_unique_params;

/* The argument checks of the uniqueness calls without a device; sgm may be NULL. */
int ws_validate_unique(const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_image *left,
                       const ws_image *right);
/* Host only: the device memory such a call would hold (sgm == NULL: ws_sgm_scratch_bytes without the sum plane). */
int ws_unique_scratch_bytes(const ws_params *p, const ws_sgm_params *sgm, const ws_image *left, const ws_image *right,
                            unsigned long long *bytes);
/* On device images into a float32 device map and, if conf_dev is not NULL, a float32 confidence plane (strides in
 * floats).  Only enqueues, on `stream` (NULL = the context's own). */
int ws_search_unique_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                            const ws_image *left_dev, const ws_image *right_dev, float *out_dev, int out_stride, float *conf_dev,
                            int conf_stride, void *stream);
/* On host buffers, synchronous, as ws_search_sgm_host; conf (float32, conf_stride floats per row) may be NULL. */
int ws_search_unique_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                          const ws_image *left, const ws_image *right, void *out, int out_stride, int out_dtype, float *conf,
                          int conf_stride);
/* {failed nodes, nodes} of the last uniqueness call of this context; waits for that call's stream. */
int ws_last_unique_counts(ws_context *ctx, unsigned long long counts[2]);

/* ---- both views from one volume (extension) ------------------------------------------------- */
/*
 * Both views' maps, and their left-right check, from the sums of ONE view: S(p, d) of the base view already holds a
 * cost for every pair (left column, right column) of a row, so the other view's map is the minimum of the same sums
 * read along the diagonal x -+ d (Hirschmueller; OpenCV's disp2 / disp12MaxDiff).  p, K(p), C, nodes, S and the
 * fallbacks are those of the SGM and uniqueness sections.  p->view names the BASE VIEW.  sgm may be NULL: S = C, the
 * uniqueness calls' block route.
 *   1. Base map: what the library already computes, bit for bit, the sub-pixel map included.  With uq given it is
 *      ws_search_unique_*'s map; with sgm given and uq NULL, ws_search_sgm_*'s; with both NULL, ws_search_*'s at
 *      smoothFactor 1.
 *   2. Derived map, base LEFT (d = 1 + j): w2 x h2, in the right view's convention.  The candidates of (y, x_r) are the d
 *      for which x = x_r + d < w1, (y, x) is a node of the base view and d is in K(y, x).  The value is the d that
 *      minimises S((y, x_r + d), d); ties take the smallest d.  It is stored as (float)d.
 *   3. Derived map, base RIGHT (d = minD + j): w1 x h1, in the left view's convention.  The candidates of (y, x_l) are the
 *      d for which 0 <= x = x_l - d < w2, (y, x) is a node and d is in K(y, x); ties take the largest d.
 *   4. No candidate: a derived pixel without candidates stores 0.0f ("no disparity"), every row beyond the base map's
 *      rows included.  With base RIGHT and minD = 0 a winner d = 0 also stores 0.0f, as the direct right map does.  The
 *      check's rule 1 reads both as empty.
 *   5. The derived map is integer-valued: it does not depend on p->subpixel, nor on uq -- every node's sums take part,
 *      whether or not the base pixel fails the ratio test.
 *   6. The check: with lr given, the two outputs are exactly what ws_lr_check_device makes of the two raw maps (base and
 *      derived, each in its own view's slot), and ws_last_lr_counts reports that check's counts.  With uq given,
 *      ws_last_unique_counts reports the base winner's counts.  With lr NULL the outputs are the raw maps.
 *   7. Identity: sgm == NULL and sgm = {paths, 0, 0} give the same two maps (S = paths * C).
 *   8. Refusals, without a device: everything ws_validate_unique refuses, with uq allowed to be NULL; what the left-right
 *      check refuses of lr, when lr is given; WS_ERR_ARG for a null output, a stride below its map's width, or
 *      overlapping outputs.
 * The derived map is not the other view's searched map: its windows are the base view's, so the two differ on some
 * pixels.  out_left is always w1 x h1 and out_right always w2 x h2, whichever view is the base.  The volumes and both
 * winners use the SGM calls' scratch, the raw maps and the check the left-right check's; a call takes the two leases in
 * that order.  The sgm == NULL route writes the whole cost plane: for the plain block search ws_search_lr_* (two
 * marching searches) stays the fast route.
 */
int ws_validate_pair(const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq, const ws_lr_params *lr,
                     const ws_image *left, const ws_image *right);
/* On device images into two float32 device maps (strides in floats).  Only enqueues, on `stream` (NULL = the context's own). */
int ws_search_pair_device(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                          const ws_lr_params *lr, const ws_image *left_dev, const ws_image *right_dev, float *out_left_dev,
                          int out_lstride, float *out_right_dev, int out_rstride, void *stream);
/* On host buffers, synchronous, as ws_search_lr_host: the images go up once, both maps come down as out_dtype (F64: the
 * float32 map widened).  Strides in elements. */
int ws_search_pair_host(ws_context *ctx, const ws_params *p, const ws_sgm_params *sgm, const ws_unique_params *uq,
                        const ws_lr_params *lr, const ws_image *left, const ws_image *right, void *out_left, int out_lstride,
                        void *out_right, int out_rstride, int out_dtype);

/* ---- census-transform matching cost (extension) -------------------------------------------- */
/*
 * WS_COST_CENSUS_5X5 / WS_COST_CENSUS_9X7 as ws_params.cost: the block search, and semi-global matching over it, on a
 * cost that does not assume both cameras see the same brightness.
 *   1. Grey: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14, in integers (14-bit BT.601; the weights sum to 16384, so a grey
 *      pixel B = G = R = v has Y = v exactly).  No bit-identity with any OpenCV release is claimed.
 *   2. Descriptor: T(y, x) lists the neighbours (y + dy, x + dx), dy = -ry .. ry outermost, dx = -rx .. rx innermost, the
 *      centre skipped; bit k (least significant first) belongs to the k-th neighbour and is 1 iff that neighbour lies
 *      inside the image and Y(neighbour) < Y(centre).  A neighbour outside the image gives 0.  Each image is
 *      transformed whole, at its own size, whatever the view.  The 5x5 descriptor sits in the low 24 bits.
 *   3. Pixel term: popcount(T_L(y, x_l) xor T_R(y, x_r)) replaces the SSD / SAD term between L(y, x_l) and R(y, x_r).
 *   4. Everything else is the block search at smoothFactor 1: the candidate sets K(p), the windows, the black test on
 *      the view's own BGR pixel, the fallbacks (x / -x / 0) and the tie rules (left view the largest d, right view the
 *      smallest) are unchanged.  C(p, d) is the integer sum of the pixel term over the window the SGM section defines
 *      (left view the full block, right view the clipped (left + right) x (up + down) window);
 *      C <= bits * block_size^2 with bits = 24 or 62, at most 62 * 63^2 = 246078.
 *   5. Sub-pixel: the parabola of the SGM section on the integer C, with the same float32 rounding.
 *   6. ws_search_sgm_* takes the census costs with no other rule changed; costs are stored in 16 bits when
 *      bits * block_size^2 <= 65535 (9x7 up to block_size 31, 5x5 up to 51).  The identity holds: with P1 = P2 = 0 the SGM
 *      map equals the census block search bit for bit, the sub-pixel map included.
 *   7. Refusals (ws_validate / ws_validate_sgm, without a device): a census cost with smooth_factor != 1, or with var_block
 *      in the right view, is WS_ERR_UNSUPPORTED; every other refusal keeps its code; WS_VIEW_LINEAR ignores cost.
 *   8. Invariance: on grey images, applying one strictly increasing map of 0..255 to either image changes no descriptor
 *      (rules 1-3), hence no map.
 * A census call is never cut into row bands (a descriptor looks ry rows beyond the window's halo): ws_search_host
 * searches it whole, and a batch with a census job is dealt as whole pairs.  Its map crosses PCIe as float32.
 *
 * The descriptors on their own: out holds h x w elements, out_stride elements apart (>= width), always 64 bits wide.  A
 * cost that is not a census value is WS_ERR_ARG.  The device form only enqueues, on `stream` (NULL = the context's own).
 */
int ws_census_transform_device(ws_context *ctx, const ws_image *img_dev, int cost, uint64_t *out_dev, int out_stride,
                               void *stream);
int ws_census_transform_host(ws_context *ctx, const ws_image *img, int cost, uint64_t *out, int out_stride);

/* ---- many pairs over the devices of a node ------------------------------------------------ */
/*
 * Independent pairs are dealt to WORKERS: one ws_context and one host thread each.  Workers are device indices; a device
 * may repeat (several contexts then share it).  Each worker runs its items as ws_enqueue_host runs pairs (two in
 * flight on its context) and ends with ws_wait.  Every map is bit-identical to ws_search_host of that pair on one
 * context, for both out_dtypes and both wire formats.  The assignment restates stereo_reconstruction_amd/sharding.py:
 *   whole pairs (bands == 0, or a batch that cannot be banded): lpt_assign, cost out_w * out_h * nd with
 *     nd = max_disparity (LEFT), max_disparity - min_disparity (RIGHT), linear_range (LINEAR);
 *   row bands (bands == 1): band_items, if every job is LEFT or RIGHT with smoothFactor 1, no varBlock, no census cost,
 *     equal image heights, and all jobs share block_size and nd (>= 1).  A band is the search of the sub-images
 *     [max(0, y0 - half), min(h, y1 + half)); only its map rows [y0, y1) are written to `out`.
 */
#define WS_JOB_NOT_RUN 1 /* ws_job.status: its worker stopped at an earlier error (or another job was invalid) */

typedef struct ws_batch ws_batch; /* not to be shared between threads (like ws_context); not usable in a forked child */

typedef struct { /* one pair: what ws_enqueue_host takes, plus its outcome */
    ws_params params;
    ws_image left, right; /* host buffers */
    void *out;            /* the map: out_h x out_w elements of out_dtype, out_stride elements apart */
    int out_stride;
    int out_dtype;
    int status; /* out: WS_OK, a WS_ERR_*, or WS_JOB_NOT_RUN */
} ws_job;

typedef struct { int job, y0, y1, worker; } ws_batch_item; /* map rows [y0, y1) of job `job`, searched on worker `worker` */

/*
 * devices: n_workers device indices (a device may repeat); NULL = one worker per device of ws_device_count() (n_workers
 * is then ignored).  Creates the workers' contexts.  Message of a failure via ws_batch_last_error(NULL).
 */
int ws_batch_create(const int *devices, int n_workers, ws_batch **out);
void ws_batch_destroy(ws_batch *b);
/* Text of the last error of this batch (b == NULL: of the last failed ws_batch_create / ws_batch_plan on this thread). */
const char *ws_batch_last_error(const ws_batch *b);
int ws_batch_workers(const ws_batch *b, int *devices, int cap); /* the workers' devices; returns their count */
/*
 * Host only, no device: the items a batch call with n_workers workers would run, grouped by worker.  Checks the jobs'
 * parameters and images as ws_validate does (not their `out`).  *n_items = the number of items (at most
 * n_jobs + n_workers - 1); WS_ERR_ARG if that exceeds cap.  *banded = 1 if the batch was cut into row bands.
 */
int ws_batch_plan(const ws_job *jobs, int n_jobs, int n_workers, int bands, int min_rows, ws_batch_item *items, int cap,
                  int *n_items, int *banded);
/*
 * Synchronous: every map is in its `out` on return.  Every job is checked first, with the checks of ws_enqueue_host; if
 * any is invalid, nothing is searched, no `out` is written, the call returns the status of the lowest-index invalid job
 * and the message names it.  A worker that meets an error stops: its remaining items are not run, the other workers
 * finish theirs.  Each job's status is set; the call returns the error of the lowest-index job that has one.
 * bands: 0 = whole pairs, 1 = row bands where the batch allows them; min_rows >= 1 (bands keep at least that many rows).
 */
int ws_batch_search_host(ws_batch *b, ws_job *jobs, int n_jobs, int bands, int min_rows);

/* ---- consumers of the map: the Reconstruction side of the call surface ------------------- */
/*
 * removeDisparityOutliers(disparityMap, kernelSize, thrFront, thrBack)  (reconstruction.cpp:5-18,
 * main.cpp:53): k x k cv::blur (normalised box, BORDER_REFLECT_101), then every value above
 * thrFront * blurred or below thrBack * blurred is replaced by the blurred one.  In place, float32.
 */
int ws_remove_disparity_outliers(ws_context *ctx, float *map, int width, int height, int stride,
                                 int kernel_size, float thr_front, float thr_back);
/* convertDisparityToDepth(dispImage, focalLength, baseline)  (reconstruction.cpp:30-43): f*b/d, 0 -> -inf */
int ws_convert_disparity_to_depth(ws_context *ctx, const float *disp, int width, int height, int stride,
                                  float focal_length, float baseline, float *depth, int depth_stride);
/*
 * The back-projection loop of reconstruction() (reconstruction.cpp:152-196): positions = w*h x 4
 * floats (x_cam, y_cam, depth, 1; all -inf where depth is -inf), colors = w*h x 4 bytes (R,G,B,255).
 * intrinsics = row-major 3x3 (fx, 0, cx, 0, fy, cy, ...).
 */
int ws_back_project(ws_context *ctx, const float *depth, int width, int height, int stride,
                    const float intrinsics[9], const ws_image *bgr, float *positions, uint8_t *colors);
/*
 * WriteMesh (reconstruction.cpp:72-149) with CheckTriangularValidity (:46-69): COFF text file -- "COFF", "<w*h> <faces> 0",
 * one line per vertex ("0 0 0 r g b a" where x is -inf, else "x y z r g b a", floats as `std::ostream << float`, i.e.
 * printf "%g"), then "3 a b c" for every triangle (i00, i10, i01), (i10, i11, i01) of every grid cell, row-major, whose
 * three corners are valid and whose edges are all at most edge_threshold long.  This one runs on the host and is what
 * the device form below is tested against.
 */
int ws_write_mesh_off(const char *path, const float *positions, const uint8_t *colors, int width,
                      int height, float edge_threshold);
/*
 * The same file, byte for byte, from vertex buffers in device memory (the layout ws_back_project writes: positions
 * w*h x 4 floats, 16-byte aligned; colors w*h x 4 bytes, 4-byte aligned).  Kernels test the triangles, format every line
 * and lay the text out; the host only moves the finished bytes into the file, in bounded chunks through pinned memory
 * of the context.  Orders after `stream` (NULL = the context's own) and returns once the file is written and closed.
 * WS_ERR_IO if the path cannot be opened (before any device work) or a write fails; WS_ERR_ARG for null pointers,
 * sizes < 1 or w*h beyond 32-bit vertex indices (UINT32_MAX).
 */
int ws_write_mesh_off_device(ws_context *ctx, const float *positions_dev, const uint8_t *colors_dev, int width,
                             int height, float edge_threshold, const char *path, void *stream);
/*
 * reconstruction(bgrImage, depthValues, intrinsics, thrMesh) (reconstruction.cpp:152-208, main.cpp:64) in one
 * synchronous call: depth and BGR image go up, the vertices are built on the device (as ws_back_project builds them)
 * and stay there, the mesh text is built by the kernels of ws_write_mesh_off_device and only the text comes down.  The
 * file is byte-identical to ws_back_project followed by ws_write_mesh_off.  Errors as ws_write_mesh_off_device.
 */
int ws_reconstruction_host(ws_context *ctx, const float *depth, int width, int height, int stride,
                           const float intrinsics[9], const ws_image *bgr, float edge_threshold, const char *path);

/* ---- measurement ------------------------------------------------------------------ */
/* hipEvent pair on `stream` (NULL = context stream): begin, enqueue work, end -> elapsed ms. */
int ws_timer_begin(ws_context *ctx, void *stream);
int ws_timer_end(ws_context *ctx, void *stream, float *elapsed_ms);
/*
 * With profiling on, every ws_search_* call brackets its dominant kernel (the marching
 * kernel) with a hipEvent pair on the launch stream; ws_last_kernel_ms waits for it and
 * returns that one launch's duration.  This is what bench.py's `roofline` is computed from.
 */
int ws_set_profiling(ws_context *ctx, int enable);
int ws_last_kernel_ms(ws_context *ctx, float *elapsed_ms);
/*
 * What the reference prints as "max block size" after computeDisparityMapRight
 * (BlockSearch.cpp:177): the largest block varBlock grew to in the last right-view call of this
 * context (block_size itself if nothing grew or varBlock was off).  Synchronises the device.
 */
int ws_last_max_block(ws_context *ctx, int block_size, int *max_block);
/*
 * After a ws_search_* call: the kernel that dominates it and how the path was tiled
 * (name as it appears in a rocprofv3 kernel trace, threads per workgroup, workgroups,
 * dynamic LDS bytes).  For reports; not part of the reference's surface.
 */
int ws_last_launch_info(const ws_context *ctx, char *kernel_name, int name_cap,
                        int *threads, int *workgroups, int *lds_bytes);
/* Tuning knob for the LDS tile sweep of BASELINE.json config 3: 0 = automatic. */
int ws_set_tuning(ws_context *ctx, int x_runs_per_tile, int strip_rows, int threads);
/*
 * ws_search_host cuts a big call into row bands whose host<->device copies overlap the searches of their
 * neighbours (smoothFactor 1, equal image heights; results are identical: each row only depends on the rows
 * under its window, BlockSearch.cpp:46-66).  bands: -1 = automatic (4 for maps of a megapixel or more),
 * 0 or 1 = never, 2..8 = that many.  For measurements; not part of the reference's surface.
 */
int ws_set_host_bands(ws_context *ctx, int bands);
/*
 * ws_search_device only enqueues.  This waits for `stream` (NULL: the context's) and returns what the kernels
 * flagged since the last check: WS_ERR_HIP if a band of the left view's smoothFactor raster pass
 * (BlockSearch.cpp:68-73 in raster order) gave up waiting for the band above it -- the map is then not valid --
 * else WS_OK.  The host entry points (ws_search_host, ws_wait) make the same check themselves.
 */
int ws_device_status(ws_context *ctx, void *stream);
/*
 * How the bytes of the last host call's three buffers (left, right, out; for a batch: of its last pair) crossed:
 * 0 = not a linear span (gathered rows), 2 = memory the caller (or a framework) had pinned already, used as it is,
 * 3 = through pinned staging memory of the library (pageable memory always does: this library registers no caller
 * memory).  (1 = registered by this library: rounds 2-3 only, never returned any more.)
 * Stands in for nothing in the reference (cv::Mat buffers are pageable and rectification.cpp:66-88 never leaves the
 * host); for tests and reports.
 */
int ws_last_host_paths(const ws_context *ctx, int how[3]);
/*
 * The format the last ws_search_host call's map crossed PCIe in: 1 = 16-bit integers (every value a search stores is
 * an integer in [-width, max(maxDisparity, width)], BlockSearch.cpp:33,82,174 -- taken whenever those bounds fit 16
 * bits and the search kernels write the map themselves: smoothFactor 1, no sub-pixel refine, no varBlock), widened to
 * the caller's CV_32F / CV_64F on the host inside the copy out of the staging memory; 2 = float32.  Doubles never
 * cross.  The map the caller gets is the same either way; for tests and reports.
 */
int ws_last_wire_format(const ws_context *ctx, int *wire);
/*
 * Which kernels the last ws_remove_disparity_outliers call ran: 0 = the double-precision box filter, 1 = the 32-bit
 * integer one (every value of the map an integer in [0, 255] and kernel_size <= 4000: what reconstruction.cpp:5-18 is
 * fed by main.cpp:47-53, an 8-bit PNG blurred over 500 x 500), 2 = the integer one met another value, left the map
 * alone, and the double one ran after it.  The results are identical; for tests and reports.
 */
int ws_last_outliers_path(const ws_context *ctx, int *path);
/*
 * Which form of those kernels the last ws_remove_disparity_outliers call launched, recorded by the launchers at the
 * launch: integer_pass for the 32-bit integer box filter, double_pass for the double-precision one (both are filled
 * when ws_last_outliers_path is 2; a pass that did not run is all zeros).
 *   row_kernel  0 = not launched, 1 = 32-bit integer rows, 2 = double rows with the row's prefix in LDS,
 *               3 = the direct O(kernel_size) rows (width > 5458)
 *   row_passes  trips of the row kernel's loading loop: 4096 pixels a trip for 1, 2048 for 2, 0 for 3
 *   row_per     pixels per thread of row kernel 2's scan, ceil(width / 256); 0 for the others
 *   col_band    columns per workgroup of the column kernel (integer: 4, 8, 16; double: 2, 4, 8, 16);
 *               0 = the direct O(kernel_size) columns (double only, height > 9087)
 *   row_window  1 = short (kernel_size <= width: the window reflects once at most), 2 = periodic
 *   col_window  the same for kernel_size and height
 * The results do not depend on the form; for tests and reports.
 */
typedef struct ws_outliers_pass {
    int row_kernel, row_passes, row_per, col_band, row_window, col_window;
} ws_outliers_pass;
typedef struct ws_outliers_forms {
    ws_outliers_pass integer_pass, double_pass;
} ws_outliers_forms;
int ws_last_outliers_forms(const ws_context *ctx, ws_outliers_forms *forms);

/* ---- Middlebury plumbing around the path ------------------------------------------ */
/*
 * PFM ("Pf", one channel): replaces the Middlebury SDK ReadImageVerb the reference uses for
 * disp0GT.pfm (data_loader.cpp:110-125).  Rows are returned top-to-bottom; unknown = +inf.
 * ws_pfm_read allocates *data with malloc (release with ws_free).
 */
int ws_pfm_read(const char *path, float **data, int *width, int *height);
int ws_pfm_write(const char *path, const float *data, int width, int height, int stride);
void ws_free(void *p);
/*
 * Binary PPM ("P6") <-> BGR rows: stands in for cv::imread(IMREAD_COLOR) / cv::imwrite of the
 * reference's PNG pairs (data_loader.cpp:71-72); no PNG codec is linked.  ws_ppm_read allocates
 * *bgr with malloc (release with ws_free).
 */
int ws_ppm_read(const char *path, uint8_t **bgr, int *width, int *height);
int ws_ppm_write(const char *path, const uint8_t *bgr, int width, int height, int stride);
/*
 * calib.txt: cam0 / cam1 as the reference parses them (data_loader.cpp:141-164), row-major
 * 3x3 each, plus the keys it leaves unread (ndisp, doffs, baseline, width, height; -1 if absent).
 */
typedef struct {
    float cam0[9];
    float cam1[9];
    float doffs, baseline;
    int width, height, ndisp;
} ws_calib;
int ws_calib_read(const char *path, ws_calib *out);
/*
 * evaldisp (utils.cpp:123-168): the bad-pixel metric ("bad-2.0" = badthresh 2.0).
 * res[0]=n, res[1]=bad %, res[2]=invalid %, res[3]=total bad %, res[4]=avgErr, res[5]=valid %.
 */
int ws_evaldisp(const float *disp, const float *gt, const uint8_t *mask, int width,
                int height, float badthresh, float maxdisp, int rounddisp, double res[6]);

#ifdef __cplusplus
}
#endif
#endif /* WS_STEREO_H */
