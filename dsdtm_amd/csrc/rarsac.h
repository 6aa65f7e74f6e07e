// rarsac.h — launch-side declarations shared by rarsac.hip and rarsac_api.cpp (libdsdtm_amd_rarsac.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_rarsac.h"

namespace dsdtm {

constexpr int RARSAC_ROUND = 256;                         // hypotheses per round = threads of the workgroup (lane = hypothesis)
constexpr int RARSAC_GRID = DSDTM_RARSAC_GRID;

// What the host derives from a desc while it checks it (R1, R2 and the weights of R3), as the kernel reads it
struct RarsacTable {
    double prior[RARSAC_GRID];         // grid_probability_in
    double binp[RARSAC_GRID];          // R2
    int32_t start[RARSAC_GRID + 1];    // the sorted correspondences of bin j: start[j] .. start[j + 1]
    int32_t nbin[RARSAC_GRID];         // the non-empty bins in bin order ...
    int32_t cum[RARSAC_GRID];          // ... and the inclusive prefix sums of their weights
    int32_t pad;
};

// One problem as the kernel sees it (an array of these is the head of the uploaded block; the host checked every field)
struct RarsacDev {
    const float* pt;                   // device, m x 4 (cur x, cur y, prev x, prev y), SORTED BY BIN (stable), 16-byte aligned
    const RarsacTable* table;          // device
    uint8_t* status;                   // device, m bytes, in sorted positions (the host puts them back)
    dsdtm_rarsac_result* out;          // device; found is always written, the rest only with found = 1
    double terminate;
    float inv_sigma2;                  // R5's invSigmaSquare
    float F[9];                        // check only
    uint32_t seed;
    int32_t m, nb, total, gr, gc, max_iterations;
    int32_t check;                     // 1: R5-R6 alone for F (dsdtm_rarsac_check)
    int32_t pad;
};

// ONE launch: workgroup p solves problem p.
hipError_t rarsac_launch(const RarsacDev* recs, int n, hipStream_t stream);

}  // namespace dsdtm
