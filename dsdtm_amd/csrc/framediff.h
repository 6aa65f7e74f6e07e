// framediff.h — launch-side declarations shared by framediff.hip and framediff_api.cpp (libdsdtm_amd_framediff.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_framediff.h"

namespace dsdtm {

// One pair of dsdtm_framediff_steps / one image of dsdtm_framediff_warp as the kernels see it: every pointer is a DEVICE address (the
// upload, the read-back part of the block, the caller's device array, or the device view of the caller's pinned array).
struct FrameDiffDev {
    double M[9];                      // F1
    const uint8_t* a;                 // NULL: the warp alone (framediff_warp_kernel reads b only)
    const uint8_t* b;
    uint8_t* mask;                    // NULL: not written (no feature asked either)
    uint8_t* warped;                  // NULL: not wanted
    const float* feat;                // n_feat x 2
    uint8_t* flags;                   // n_feat
    int32_t* n_foreground;            // one counter, zero when the launch starts
    int32_t w, h, a_stride, b_stride, mask_stride, warped_stride;
    int32_t threshold, maxval, n_feat, reserved;
};

// R: the rows of one image a workgroup owns (at full width). It evaluates F2-F5 for R + 12 rows, 6 halo rows either side (2 per pass of
// F6), so the recompute overhead is (R + 12) / R: 1.375 at 32. Chosen by measurement against 16 (profiles/r25_framediff.txt: 16 is 11-15 us faster
// for one pair, 32 is 14-17 % faster per pair in batches of 64 and 1024 with the mask left on the device).
#ifndef FRAMEDIFF_ROWS
#define FRAMEDIFF_ROWS 32
#endif
enum { FRAMEDIFF_HALO = 6, FRAMEDIFF_THREADS = 1024 };      // 16 wavefronts: one pair is few bands, and a band's words are its parallelism

// F2-F7 (and the counter of F8) for n pairs in ONE launch: grid (ceil(max_h / R), n), 2 bit-planes of (R + 12) x ceil(max_w / 64) words
// of dynamic LDS. No workgroup waits for another.
hipError_t framediff_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream);
// F8's flags against the mask where it lies: grid (ceil(max_features / 256), n)
hipError_t framediff_features_launch(const FrameDiffDev* recs, int n, int max_features, hipStream_t stream);
// F2-F3 alone, b -> warped: grid (ceil(max_w / 64), ceil(max_h / 4), n)
hipError_t framediff_warp_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream);

}  // namespace dsdtm
