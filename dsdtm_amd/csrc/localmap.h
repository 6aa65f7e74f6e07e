// localmap.h — launch-side declarations shared by localmap.hip and localmap_api.cpp (libdsdtm_amd_localmap.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_localmap.h"

namespace dsdtm {

// What a map's device arrays start with (elements); each doubles, up to its limit, when an update needs more.
constexpr int LM_INITIAL_POINTS = 4096;
constexpr int LM_INITIAL_KEYFRAMES = 64;
constexpr int64_t LM_INITIAL_SLOTS = 16384;

// A map point on the device: 32 bytes, so that one aligned 32-byte read brings the position the visibility test gathers.
struct LmPointDev {
    double x, y, z;
    uint64_t bad;               // IsBad(): 0 / 1
};
// A keyframe on the device: its slots are slots[slot_off .. slot_off + n_slots) of the map's slot pool.
struct LmKeyframeDev {
    double T[12];
    int64_t slot_off;
    int32_t n_slots, reserved;
};

// An update as the device sees it: up to two runs of 32-bit words copied from the staging block into the map's arrays by ONE
// launch (a keyframe's record and its slots change together or not at all).
struct LmApplyArgs {
    uint32_t* dst[2];
    const uint32_t* src[2];
    uint32_t words[2];
};
hipError_t localmap_apply_launch(const LmApplyArgs& args, hipStream_t stream);

// One desc of dsdtm_localmap_select on the device. keys and the outputs lie in the call's device block at these byte offsets
// (8-aligned): keys K x 8; kf_dist n_local x 8; result 16; kf n_local x 4; point and point_kf capacity x 4 each.
struct LmDescDev {
    double T[12];
    const LmPointDev* points;
    const LmKeyframeDev* kfs;
    const int32_t* slots;
    int32_t K, P;               // keyframes and points of the map at the time of the call
    int32_t capacity, reserved;
    uint64_t keys, kf_dist, result, kf, point, point_kf;
};
struct LmSelectArgs {
    uint8_t* block;             // device: n descs, then what their offsets address
    int n, max_K, max_P;        // the largest K and P among the descs: the grid of the first kernel, the bitmap of the second
    int n_local, boundary;      // 1 .. DSDTM_LOCALMAP_MAX_LOCAL, >= 0 (the host checked)
    float fx, fy, cx, cy;
    int width, height;
};
// The two launches of a select: keys (one wavefront per desc and keyframe), then selection and walk (one workgroup per desc).
hipError_t localmap_select_launch(const LmSelectArgs& args, hipStream_t stream);

}  // namespace dsdtm
