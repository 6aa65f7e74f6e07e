// keyframe.h — launch-side declarations shared by keyframe.hip and keyframe_api.cpp (libdsdtm_amd_keyframe.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_keyframe.h"

namespace dsdtm {

// Tracking::NeedKeyframe (src/Tracking.cpp:347-410) for n trackers: one wavefront (= one workgroup) per tracker (keyframe.hip).
// A tracker's arrays lie in one blob (the upload of dsdtm_need_keyframes) at the byte offsets of its record, 8-aligned.
struct KeyframeTrackerDev {
    double T_cur[12], T_kf[12];
    int32_t n_valid, n_cur, n_kf, n_lkf;        // n_cur, n_kf <= DSDTM_KF_MAX_POINTS, n_lkf <= DSDTM_KF_MAX_LOCAL_KF (the host checked)
    uint64_t cur_p, cur_bad, kf_p, kf_bad, lkf; // doubles n_cur x 3, bytes n_cur, doubles n_kf x 3, bytes n_kf, doubles n_lkf x 3
};
struct KeyframeArgs {
    const uint8_t* blob;                        // device: n records, then their arrays
    dsdtm_keyframe_verdict* verdict;            // device: n
    int n;
    float fx, fy, cx, cy;
    dsdtm_keyframe_params prm;                  // px_samples in 1..64 (the host checked)
};
hipError_t need_keyframes_launch(const KeyframeArgs& args, hipStream_t stream);

}  // namespace dsdtm
