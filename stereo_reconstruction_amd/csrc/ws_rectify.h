// ws_rectify.h -- launch interface of the image rectification kernel (ws_rectify.hip) for the C-ABI host code
// (ws_capi.cpp).  Internal; the public boundary is include/ws_stereo.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wsamd {

// cv::warpPerspective(src, dst, M, dst.size()) -- INTER_LINEAR, BORDER_CONSTANT 0 -- of a CV_8UC3 image.
// minv = M^-1 (destination -> source, row-major).  src: sh rows of 3*sw bytes, sp bytes apart; the kernel reads no
// byte outside [src, src + sp*(sh-1) + 3*sw).  dst: dh rows of 3*dw bytes, dp bytes apart.
hipError_t launch_rectify(const uint8_t *src, int sw, int sh, int sp, const double minv[9], uint8_t *dst, int dw, int dh,
                          int dp, hipStream_t s);

} // namespace wsamd
