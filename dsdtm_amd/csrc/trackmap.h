// trackmap.h — launch-side declarations shared by trackmap.hip and trackmap_api.cpp (libdsdtm_amd_trackmap.so). The selection is the two
// launches of localmap.hip (localmap.h), which this library links as they are: the map's point, keyframe and slot arrays keep the
// LmPointDev / LmKeyframeDev / int32 layout, so that an LmDescDev addresses them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_trackmap.h"
#include "localmap.h"

namespace dsdtm {

// The observing feature of a slot: 40 bytes, copied to the outputs as it is.
struct TmFeatDev {
    float px[2];                // Feature::mpx
    int32_t level, reserved;    // Feature::mlevel
    double bearing[3];          // Feature::mNormal
};

// An update as the device sees it: up to four runs of 32-bit words copied from the staging block into the map's arrays by ONE launch
// (a keyframe's record, its slots, their flags and their features change together or not at all).
struct TmApplyArgs {
    uint32_t* dst[4];
    const uint32_t* src[4];
    uint32_t words[4];
};
hipError_t trackmap_apply_launch(const TmApplyArgs& args, hipStream_t stream);

// points_write: n points from `first` on. bad / found NULL: zero for a point at or behind old_count (an append), unchanged below it.
struct TmPointsArgs {
    LmPointDev* points;
    int32_t* found_dst;
    const double* xyz;          // staged: n x 3
    const uint8_t* bad;         // staged: n, or NULL
    const int32_t* found;       // staged: n, or NULL
    int32_t first, n, old_count, reserved;
};
hipError_t trackmap_points_launch(const TmPointsArgs& args, hipStream_t stream);
// found_write: found_dst[index[i]] = found[i] (the host checked the indices: in range, no duplicates)
hipError_t trackmap_found_launch(int32_t* found_dst, const int32_t* index, const int32_t* found, int n, hipStream_t stream);

// What the flatten leaves per desc beside the selection's dsdtm_localmap_result
struct TmExtResult {
    int32_t n_obs, overflow_obs;
    int32_t straddle;           // the emitted point whose segment crosses obs_capacity, or -1
    int32_t reserved;
};
// One desc of dsdtm_trackmap_local on the device, beside the LmDescDev of the same index (which has the pose, the point / keyframe / slot
// arrays, K, P, point_capacity and the selection's outputs). Byte offsets into the call's device block, 8-aligned.
struct TmDescDev {
    const int32_t* found;       // per point
    const int32_t* obs;         // per slot of the pool: the point index when the slot observes, -1 otherwise
    const TmFeatDev* feat;      // per slot of the pool
    int32_t ocap, reserved;     // obs_capacity
    uint64_t ext;               // TmExtResult
    uint64_t mp_world, mp_found, mp_bad, obs_offset;            // capacity x 24, x 4, x 1, (capacity + 1) x 4
    uint64_t obs_kf, obs_px, obs_level, obs_bearing;            // ocap x 4, x 8, x 4, x 24
    uint64_t count, cursor, pairs;                              // not read back: capacity x 4 each, ocap x 8 ((keyframe << 32) | slot)
};
struct TmLocalArgs {
    uint8_t* block;             // device: n LmDescDev, then n TmDescDev at `descs`, then what their offsets address
    uint64_t descs;
    int n, max_K, max_cap, max_ocap;       // the largest K, point_capacity and obs_capacity among the descs: the grids
};
// The launches of the flatten, behind localmap_select_launch on the same stream: gather, count, scan, fill, straddle, emit.
hipError_t trackmap_flatten_launch(const TmLocalArgs& args, hipStream_t stream);

}  // namespace dsdtm
