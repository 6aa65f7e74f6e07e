// example_mapping.cpp — the mapping thread on the resident map (include/dsdtm_amd_mapping.h): a new keyframe's
// covisibility list, then one local bundle adjustment as window -> solve -> commit with no column crossing the link, and the host
// evaluation of the same window for comparison. Device memory is the caller's (here: hipMalloc'ed by whoever links this).
//
//   hipcc -std=c++17 example_mapping.cpp -L../csrc -ldsdtm_amd_mapping -ldsdtm_amd        (the compiler sees it in tests/test_ba_window_cpu.py)
#include <cstdio>

#include "dsdtm_mapping_host.hpp"

// One mapping step for keyframe `kf` of the map `mapping` holds. `arrays`, `d_outlier`, `d_summary`: device memory sized by the capacities.
int MappingStep(DSDTM::Mapping& mapping, dsdtm_ctx* solver, int32_t kf, int32_t origin_kf, const dsdtm_mapping_window_arrays& arrays, uint8_t* d_outlier,
                dsdtm_local_ba_summary* d_summary, void* hip_stream) {
    // KeyFrame::UpdateConnection, when the keyframe is created: the stored GetCovKFrames()
    int32_t n_connected = 0;
    std::vector<int32_t> cov_kf;
    for (const auto& weight_kf : mapping.UpdateConnectionOnDevice(kf, &n_connected)) cov_kf.push_back(weight_kf.second);
    std::printf("keyframe %d: %zu covisible keyframes of %d connected\n", kf, cov_kf.size(), n_connected);
    if (cov_kf.size() > DSDTM_MAPPING_MAX_COV) cov_kf.erase(cov_kf.begin(), cov_kf.end() - DSDTM_MAPPING_MAX_COV);       // (the strongest ones)

    dsdtm_local_ba_params params = {10, 0, 2.0 / 500.0};
    const DSDTM::Mapping::LocalBaOutcome r = mapping.LocalBundleAdjustmentOnDevice(
        solver, kf, cov_kf, origin_kf, params, arrays, DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF, DSDTM_LBA_MAX_POINTS, DSDTM_LBA_MAX_OBSERVATIONS,
        d_outlier, d_summary, hip_stream);
    if (!r.usable) {
        std::printf("window not usable (free > 16: %d, constant > 64: %d, ...): take the host path for this keyframe\n", r.window.over_free_kf, r.window.over_const_kf);
        return 1;
    }
    std::printf("window: %d local + %d fixed keyframes, %d points, %d observations; %d outliers, %d points went bad\n", r.window.n_local, r.window.n_fixed,
                r.window.n_points, r.window.n_obs, r.commit.n_outliers, r.commit.n_bad);
    return 0;
}

// The same window on the host, from a map read back (dsdtm_mapping_map_read): no library needed.
DSDTM::BaWindowHost WindowOnHost(const DSDTM::TrackMapArrays& map, int32_t kf, int32_t origin_kf) {
    const DSDTM::CovisibilityHost cov = DSDTM::update_connection_host(map, kf);
    return DSDTM::ba_window_host(map, kf, (int32_t)cov.cov_kf.size(), cov.cov_kf.data(), origin_kf, DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF,
                                 DSDTM_LBA_MAX_POINTS, DSDTM_LBA_MAX_OBSERVATIONS);
}
