// mapping.h — launch-side declarations shared by mapping.hip and mapping_api.cpp (libdsdtm_amd_mapping.so). The map is the track map of
// trackmap.h (LmPointDev, LmKeyframeDev, the slot pool with point_of_slot, the observing point and the feature record).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dsdtm_amd_mapping.h"
#include "trackmap.h"

namespace dsdtm {

// ---- dsdtm_mapping_covisibility. Byte offsets into the call's device block, 8-aligned.
struct MpCovDev {
    const LmPointDev* points;
    const LmKeyframeDev* kfs;
    const int32_t* slots;       // point_of_slot
    const int32_t* obs;         // the observing point of each slot, or -1
    int32_t K, kf, capacity, reserved;
    uint64_t weight;            // K x 4, not read back
    uint64_t cov_kf, cov_weight, result;   // capacity x 4 each, dsdtm_mapping_cov_result
};
struct MpCovArgs {
    uint8_t* block;             // n MpCovDev, then what their offsets address
    int n, max_K;
};
hipError_t mapping_covisibility_launch(const MpCovArgs& args, hipStream_t stream);

// ---- dsdtm_mapping_ba_window. An ENTRY is a slot of a local keyframe, numbered in (rank of the local keyframe, slot) order: entry e of
// local keyframe r is slot e - ent_off[r]. The first-occurrence table (open addressing, T a power of two >= 2 E: a probe always ends)
// holds (point << 32 | smallest entry that lists it).
struct MpWinDev {
    const LmPointDev* points;
    const LmKeyframeDev* kfs;
    const int32_t* slots;
    const int32_t* obs;
    const TmFeatDev* feat;
    int32_t K, P, kf, origin, n_local, E, T_bits, kcap, pcap, ocap;
    // the window's segments of the caller's device arrays
    double* T_c2w; uint8_t* kf_constant; double* pts;
    int32_t* obs_kf; int32_t* obs_point; double* obs_bearing; int32_t* obs_level;
    int32_t* kf_index; int32_t* point_index; int64_t* obs_slot;
    uint64_t result;            // dsdtm_mapping_window_result (read back)
    uint64_t local, ent_off;    // uploaded: n_local x 4, (n_local + 1) x 4
    uint64_t table, cell_lp;    // T x 8, T x 4 (the window point of the cell's point)
    uint64_t count, cursor, off;   // E x 4, E x 4, (E + 1) x 4: per window point
    uint64_t kfkey, kfwin;      // K x 4 each: the first window point a non-local keyframe observes; keyframe -> window keyframe or -1
    uint64_t pairs;             // ocap x 8
};
struct MpWinArgs {
    uint8_t* block;
    int n, max_K, max_E, max_T, max_ocap;
};
hipError_t mapping_window_launch(const MpWinArgs& args, hipStream_t stream);

// ---- dsdtm_mapping_ba_commit: one record per USABLE window.
struct MpCommitDev {
    LmPointDev* points;
    LmKeyframeDev* kfs;
    int32_t* slots;
    int32_t* obs;
    int32_t K, P, n_kf, n_points, n_obs, window, bad_cap, reserved;
    const double* T_c2w; const double* pts;
    const int32_t* obs_point; const int32_t* kf_index; const int32_t* point_index; const int64_t* obs_slot;
    const uint8_t* outlier;
    uint64_t claim_k, claim_p;  // K x 4, P x 4: of the window's MAP (shared by the windows of that map)
    uint64_t went_bad, n_out;   // n_points x 4 each
    uint64_t bad_list, result;  // bad_cap x 4, dsdtm_mapping_commit_result (read back)
};
struct MpCommitArgs {
    uint8_t* block;
    int n, max_items;           // the largest max(n_kf, n_points) among the records
    uint64_t verdict;           // 8 bytes: (first window << 32 | second window) of the smallest overlapping pair, or MP_NO_OVERLAP
    uint64_t claims;            // the claim arrays of every map, back to back behind the verdict ...
    uint64_t claim_words;       // ... this many 32-bit words, the verdict's two included
};
constexpr unsigned long long MP_NO_OVERLAP = 0x7fffffff7fffffffull;
// claim + verify: read-only on the map; the host waits for the verdict
hipError_t mapping_commit_check_launch(const MpCommitArgs& args, hipStream_t stream);
hipError_t mapping_commit_apply_launch(const MpCommitArgs& args, hipStream_t stream);

}  // namespace dsdtm
