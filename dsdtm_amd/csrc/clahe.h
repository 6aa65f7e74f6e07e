// clahe.h — launch-side declarations shared by clahe.hip and clahe_api.cpp (libdsdtm_amd_clahe.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_clahe.h"

namespace dsdtm {

// One frame of dsdtm_clahe_apply_batch as the kernels see it: every pointer is a DEVICE address (the upload, the read-back part of the
// block, the caller's device array, or the device view of the caller's pinned array). The geometry is clahe_geometry's
// (host/dsdtm_clahe_host.hpp), evaluated once on the host: the kernels divide nothing.
struct ClaheFrameDev {
    const uint8_t* src;
    uint8_t* dst;                     // NULL: tables only (dsdtm_clahe_luts)
    uint8_t* luts;                    // tiles_y * tiles_x * 256 bytes, 256-byte aligned
    int32_t w, h, src_stride, dst_stride;
    int32_t tiles_x, tiles_y, tile_w, tile_h;
    int32_t clip;                     // 0: no clipping
    float scale, inv_tw, inv_th;
};

enum {
    CLAHE_THREADS = 256,
    CLAHE_PX = 4,                                   // interpolation: a thread has 4 adjacent pixels of a row ...
    CLAHE_CHUNK = 64 * CLAHE_PX,                    // ... a wavefront 256 adjacent pixels, the workgroup's column chunk
    CLAHE_ROWS = 16,                                // rows of a workgroup (4 per wavefront), all within one (ty1, ty2) pair
    CLAHE_BANDS = DSDTM_CLAHE_MAX_TILES + 1,        // (ty1, ty2) pairs of a frame at most: tiles_y + 1
};

// E1-E5 for n frames in one launch: grid (max_tiles, n), one workgroup per (tile, frame). No launch waits for another workgroup.
hipError_t clahe_luts_launch(const ClaheFrameDev* frames, int n, int max_tiles, hipStream_t stream);
// E6 for n frames in one launch: grid (ceil(max_w / 256) * ceil(max_tile_h / 16), max_tiles_y + 1, n)
hipError_t clahe_interp_launch(const ClaheFrameDev* frames, int n, int max_w, int max_tile_h, int max_tiles_y, hipStream_t stream);

}  // namespace dsdtm
