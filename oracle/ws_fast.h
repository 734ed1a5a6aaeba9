/*
 * ws_fast.h -- fast exact CPU reference for BlockSearch (whole maps in seconds).
 *
 * TEST INFRASTRUCTURE ONLY, like ws_oracle.h.  Same results, bit for bit, as
 * wso_block_left / wso_block_right (ws_oracle.c), which re-sum every window for
 * every (pixel, disparity) pair and need minutes per full-size view.  This one
 * costs O(H * W * D) whatever the window size: exact integer column sums over
 * the window's rows, moved by one entering and one leaving row, and window sums
 * slid along x from them.  It is written along its own route on purpose, so
 * that the two restatements pin each other (tests/test_fast_reference.py).
 *
 * Images and outputs as in ws_oracle.h.  Return codes are the WSO_* codes, plus
 * WSF_ERR_UNSUPPORTED for what this reference does not implement (var_block
 * together with sub-pixel refinement, block sizes whose window sums would not
 * fit 32 bits without var_block).
 */
#ifndef WS_FAST_H
#define WS_FAST_H

#include "ws_oracle.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { WSF_ERR_UNSUPPORTED = -4 };

/* wso_block_left's semantics; threads < 1 means OpenMP's default. */
int wsf_block_left(const wso_image *L, const wso_image *R, int block_size,
                   int min_disparity, int max_disparity, double smooth,
                   int cost, int subpixel, int y0, int y1,
                   double *out, int out_stride, int threads);

/* wso_block_right's semantics without var_block (refused: WSF_ERR_UNSUPPORTED). */
int wsf_block_right(const wso_image *L, const wso_image *R, int block_size,
                    int min_disparity, int max_disparity, double smooth,
                    int var_block, int cost, int subpixel, int y0, int y1,
                    double *out, int out_stride, int threads);

/* wso_block_right's semantics, var_block, thres and max_block_out (may be NULL) included.  var_block
 * runs a route of its own (ws_fast.c): every pixel's window from a value histogram, its costs from
 * one 64-bit summed-area table per disparity, O(H * W * D) whatever the windows grow to. */
int wsf_block_right_vb(const wso_image *L, const wso_image *R, int block_size,
                       int min_disparity, int max_disparity, double smooth,
                       int var_block, double thres, int cost, int subpixel, int y0, int y1,
                       double *out, int out_stride, int *max_block_out, int threads);

#ifdef __cplusplus
}
#endif
#endif
