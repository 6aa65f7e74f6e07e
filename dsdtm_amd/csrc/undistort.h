// undistort.h — launch-side declarations shared by undistort.hip and undistort_api.cpp (libdsdtm_amd_undistort.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_undistort.h"

namespace dsdtm {

// the camera and the distortion as U1 and U5 read them: the floats widened to double once, on the host
struct UndistortModel {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// One frame of dsdtm_undistort_frames as the kernel sees it: every pointer is a DEVICE address (the upload, the read-back part of the
// block, the caller's device array, or the device view of the caller's pinned array). Strides in elements of the image's type.
struct UndistortFrameDev {
    const int32_t* map;               // w * h pairs (X, Y)
    const uint8_t* gray_src; uint8_t* gray_dst;
    const uint16_t* depth_src; uint16_t* depth_dst;      // both NULL: no depth
    int32_t w, h;
    int32_t gray_src_stride, gray_dst_stride, depth_src_stride, depth_dst_stride;
};

enum { UNDISTORT_BLOCK_X = 64, UNDISTORT_BLOCK_Y = 4, UNDISTORT_PX = 4 };      // a thread: 4 adjacent pixels; a workgroup: 256 x 4 pixels

// U1 for w x h pixels into `map` (device). No launch waits for another workgroup.
hipError_t undistort_map_launch(const UndistortModel& m, int w, int h, int32_t* map, hipStream_t stream);
// U2 + U3 for n frames in one launch: grid (ceil(max_w / 256), ceil(max_h / 4), n)
hipError_t undistort_frames_launch(const UndistortFrameDev* frames, int n, int max_w, int max_h, hipStream_t stream);
// U5: px_in n x 2, skip n (never NULL), px_out n x 2, bearing n x 3 (rows of skipped pixels are not written)
hipError_t undistort_points_launch(const UndistortModel& m, float fx, float fy, float cx, float cy, int n, const float* px_in, const uint8_t* skip,
                                   float* px_out, double* bearing, hipStream_t stream);

}  // namespace dsdtm
