// aftertrack.h — launch-side declarations shared by aftertrack.hip and slam_api.cpp (libdsdtm_amd_slam.so): dsdtm_slam_track_commit. The
// map is the track map of trackmap.h (LmPointDev, the found counts, the slot pool with point_of_slot and the observing point).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_slam.h"
#include "keyframe.h"
#include "trackmap.h"

namespace dsdtm {

constexpr int AT_THREADS = 256;     // = DSDTM_SLAM_MAX_MATCHES: thread k of a map's workgroup owns match k

// One desc of dsdtm_slam_track_commit on the device. Byte offsets into the call's device block, 8-aligned.
struct AtDescDev {
    int32_t n_matches, bad_cap;     // bad_cap: the room of bad_list (min(bad_capacity, n_matches))
    uint64_t point, norm;           // uploaded: n_matches x 4, n_matches x 8
    uint64_t found_after, bad_list, result;   // read back: n_matches x 4, bad_cap x 4, dsdtm_slam_commit_result
};
// One DISTINCT map of the call: its descs are applied by one workgroup, in desc order.
struct AtMapDev {
    LmPointDev* points;
    int32_t* found;
    int32_t* slots;                 // point_of_slot
    int32_t* obs;                   // the observing point of each slot, or -1
    int64_t S;                      // slots of the pool in use
    int32_t P, n_descs;
    uint64_t desc_list;             // uploaded: n_descs x 4, the map's descs in desc order
    uint64_t stamp;                 // not read back: P bytes (rounded up to 8), 1 = the point went bad IN THIS CALL: the mark of rule T3,
                                    // distinct from `bad`; cleared by the walk itself ...
    uint64_t n_new_bad;             // ... and the count of such points (4 bytes)
};
struct AtCommitArgs {
    uint8_t* block;                 // device: n_maps AtMapDev, then n AtDescDev at `descs`, then what their offsets address
    uint64_t descs;
    int n_maps, n;                  // (n: not read by the kernels; what a checker of the block holds the maps' desc lists against)
    long long max_S;                // the largest S among the maps: the grid of the cascade
    double threshold;
};
// The two launches of a commit: the walk (one workgroup per distinct map), then the cascade over each map's slot pool.
hipError_t aftertrack_commit_launch(const AtCommitArgs& args, hipStream_t stream);

// ---- dsdtm_slam_need_keyframes: the gather in front of keyframe.hip. The call's device block starts with the n KeyframeTrackerDev of
// keyframe.h (the blob need_keyframes_launch takes), whose T_cur, n_valid, n_cur, n_lkf and offsets the host filled; the gather writes
// T_kf, n_kf and the arrays. One record per tracker at `descs`. Byte offsets into the block, 8-aligned.
struct AtGatherDev {
    const LmPointDev* points;
    const LmKeyframeDev* kfs;
    const int32_t* slots;           // point_of_slot
    int32_t P, K, kf, reserved;
    uint64_t cur_point, local_kf;   // uploaded: n_cur x 4, n_lkf x 4
};
struct AtGatherArgs {
    uint8_t* block;
    uint64_t descs;
    int n;
};
hipError_t aftertrack_gather_launch(const AtGatherArgs& args, hipStream_t stream);

}  // namespace dsdtm
