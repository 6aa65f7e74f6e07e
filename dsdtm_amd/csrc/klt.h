// klt.h — launch-side declarations shared by klt.hip and klt_api.cpp (libdsdtm_amd_klt.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_klt.h"
#include "homography.h"

namespace dsdtm {

constexpr int KLT_WAVES = 4;                       // points per 256-thread workgroup: one wavefront each
constexpr int KLT_MAX_PASSES = 7;                  // 21 x 21 = 441 window pixels over 64 lanes

// One pair of pyramids and its points as the kernel sees it (the host checked every field)
struct KltDev {
    const uint8_t* prev;               // device, two packed pyramids of one geometry
    const uint8_t* cur;
    const float* points;               // device, n_points x 2
    const float* guesses;              // device or null (the points)
    float* out_points;                 // device, n_points x 2
    uint8_t* status;                   // device, n_points
    int32_t* iterations;               // device, n_points
    float* residual;                   // device or null
    double eps2, min_eig;
    int32_t w[DSDTM_KLT_MAX_LEVELS], h[DSDTM_KLT_MAX_LEVELS], stride[DSDTM_KLT_MAX_LEVELS];
    uint32_t off[DSDTM_KLT_MAX_LEVELS];
    int32_t n_points, levels, window, max_iter;      // n_points 0: nothing is tracked (a model's first step)
};

// A level 0 on its way into a pyramid: width x height bytes from rows sstride apart to rows dstride apart
struct KltIngest {
    const uint8_t* src;
    uint8_t* dst;
    int32_t width, height, sstride, dstride;
};

// The survivors of one model, in ascending index, into its homography record: a = current, b = previous, m = their number
// (0 when fewer than min_tracked survived, which homography.hip answers with found = 0)
struct KltCompact {
    const float* prev_points;
    const float* points;
    const uint8_t* status;
    float* a;
    float* b;
    HomographyDev* rec;
    int32_t* n_tracked;
    int32_t n_points, min_tracked;
};

// ONE launch each: block (x, y) = (chunk of the largest image, image) / (KLT_WAVES points, pair) / model.
hipError_t klt_ingest_launch(const KltIngest* recs, int n, int max_width, int max_height, hipStream_t stream);
hipError_t klt_launch(const KltDev* recs, int n, int max_points, hipStream_t stream);
hipError_t klt_compact_launch(const KltCompact* recs, int n, hipStream_t stream);

}  // namespace dsdtm
