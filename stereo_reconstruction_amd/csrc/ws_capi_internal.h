// ws_capi_internal.h -- entry points of ws_capi.cpp that other sources of the library call and that are not part of the
// C-ABI.
#pragma once

#include "../../include/ws_stereo.h"

namespace wsamd {

// ws_enqueue_host for the map rows [map_row0, map_row0 + map_rows) only (map_rows < 0: the whole map); `out` points at
// where map row map_row0 lands.  Ends with ws_wait like ws_enqueue_host.
int enqueue_host_rows(ws_context *ctx, const ws_params *p, const ws_image *left, const ws_image *right, void *out,
                      int out_stride, int out_dtype, int map_row0, int map_rows);

} // namespace wsamd
