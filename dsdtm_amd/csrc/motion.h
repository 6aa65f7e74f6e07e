// motion.h — launch-side declarations shared by motion.hip and motion_api.cpp (libdsdtm_amd_motion.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_motion.h"

namespace dsdtm {

// A model on the device: two generations of the twelve arrays (m_Mean, m_Var, m_Age, m_Mean_Temp, m_Var_Temp, m_Age_Temp x 2 modes,
// each mw * mh floats, in that order). A step reads generation g and writes every entry of generation 1 - g: compensation gathers
// the OLD m_Mean / m_Var / m_Age of neighbouring cells while update overwrites them, and a step that fails leaves g as it was.
constexpr int MOTION_ARRAYS = 12;
constexpr int MOTION_TILE_CELLS = 16;                      // a workgroup owns 16 x 16 cells = 64 x 64 pixels (one thread per cell)
constexpr int MOTION_MASK_ALIGN = 16;                      // pitch of a mask in the staging block: width rounded up to this

// One model's step as the kernels see it (an array of these is the head of the uploaded block)
struct MotionStepDev {
    const uint8_t* image;      // device; NULL: an all-zero image (ProbModel::init)
    const float* src;          // generation read; NULL: all twelve arrays zero (ProbModel::init)
    float* dst;                // generation written
    uint8_t* mask;             // device, pitch mask_pitch, 4-byte aligned rows; NULL: update(NULL), nothing written
    const float* feat;         // n_feat x 2
    uint8_t* flags;            // n_feat
    double H[9];
    int32_t width, height, mw, mh;
    int32_t img_stride, mask_pitch, n_feat, reserved;
};

// ONE launch: the median, compensation and update of every model of the batch (grid.z = model); the host checked every field.
// tiles_x / tiles_y: the largest model's tile counts.
hipError_t motion_step_launch(const MotionStepDev* recs, int n, int tiles_x, int tiles_y, hipStream_t stream);
// the feature lookup behind it (grid.y = model): flags[i] = mask(cvRound(x), cvRound(y)) == 255
hipError_t motion_features_launch(const MotionStepDev* recs, int n, int max_features, hipStream_t stream);

}  // namespace dsdtm
