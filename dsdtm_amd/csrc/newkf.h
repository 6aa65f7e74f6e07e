// newkf.h — launch-side declarations shared by newkf.hip and newkf_api.cpp (libdsdtm_amd_newkf.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_newkf.h"

namespace dsdtm {

// One tracker of dsdtm_newkf_make_batch as the kernel sees it: every pointer is a DEVICE address (the upload, the caller's device
// array, or the device view of the caller's pinned array). The outputs lie in the call's read-back block; a column holds out_slots
// entries and new_p_world out_points points — what the host knows the tracker can reach at most, never more than its capacities.
struct NewkfTrackerDev {
    const float* cell_score; const int32_t* cell_x; const int32_t* cell_y; const int32_t* cell_level;    // G each
    const float* px_xy; const int32_t* level; const double* bearing;                                      // n_existing
    const uint8_t* has_point; const uint8_t* initial; const int32_t* point_index;
    const uint16_t* depth; const uint8_t* dyn;                                                           // dyn may be NULL
    int32_t depth_stride, dyn_stride;                                                                    // elements / bytes
    float inv_depth_scale;                                                                               // 1.0f / depth_scale
    int32_t n_existing, first_point_index;
    int32_t slot_cap, point_cap, bad_cap;                                                                // the caller's capacities (bad_cap < 0: no new_bad)
    int32_t out_slots, out_points;                                                                       // what the arrays below hold
    double T[12];
    int32_t* counts;                                                                                     // n_new, n_slots, n_new_points, overflow
    int32_t* o_point_of_slot; uint8_t* o_observes; float* o_px_xy; int32_t* o_level; double* o_bearing; float* o_depth;
    double* o_p_world;
};
struct NewkfArgs {
    const NewkfTrackerDev* trackers;            // device: n
    int n;
    float fx, fy, cx, cy;
    dsdtm_newkf_params prm;                     // the host checked every range
    uint8_t hw_min[128], hw_cell[128];          // the midpoint-span half-widths per |dy| of the radii min_dist and cell_size (K3)
};
hipError_t newkf_make_launch(const NewkfArgs& args, hipStream_t stream);

}  // namespace dsdtm
