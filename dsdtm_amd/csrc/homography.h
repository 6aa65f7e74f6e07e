// homography.h — launch-side declarations shared by homography.hip and homography_api.cpp (libdsdtm_amd_homography.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_homography.h"

namespace dsdtm {

constexpr int HOMOGRAPHY_ROUND = 256;                     // hypotheses per round = threads of the workgroup (lane = hypothesis)
constexpr int HOMOGRAPHY_MAX_ROUNDS = DSDTM_HOMOGRAPHY_MAX_HYPOTHESES / HOMOGRAPHY_ROUND;

// One problem as the kernel sees it (an array of these is the head of the uploaded block; the host checked every field)
struct HomographyDev {
    const float* a;                    // device, m x 2 (x, y), 8-byte aligned
    const float* b;
    uint8_t* mask;                     // device, m bytes
    dsdtm_homography_result* out;      // device; found is always written, the rest only with found = 1
    double thr2;                       // reproj_threshold squared
    double left;                       // 1.0 - confidence
    int32_t m, rounds_max;
    uint32_t seed, reserved;
};

// ONE launch: workgroup p solves problem p.
hipError_t homography_launch(const HomographyDev* recs, int n, hipStream_t stream);

}  // namespace dsdtm
