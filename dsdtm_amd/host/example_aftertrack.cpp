// example_aftertrack.cpp — a tracked frame's effects on the resident map (include/dsdtm_amd_slam.h): after
// dsdtm_slam_local and dsdtm_track_frame, one dsdtm_slam_track_commit keeps the map's found counts, bad flags and slots true for the
// next frame; and the host evaluation of the same rules for a caller whose map lives on the host.
//
//   hipcc -std=c++17 example_aftertrack.cpp -L../csrc -ldsdtm_amd_slam        (the compiler sees it in tests/test_aftertrack_cpu.py)
#include <cstdio>

#include "dsdtm_slam_host.hpp"

// The end of one tracked frame on the map `slam` holds. point_list: the `point` column dsdtm_slam_local returned for the frame;
// match_point / residual_norm: ms[k].point and the norms of dsdtm_track_frame; f: the camera's focal length.
int AfterTrackedFrame(DSDTM::Slam& slam, const std::vector<int32_t>& point_list, const std::vector<int32_t>& match_point, const std::vector<double>& residual_norm,
                      double local_ba_threshold, double f) {
    const double tOutlineThres = local_ba_threshold / f;        // src/Optimizer.cpp:22-24
    const DSDTM::Slam::TrackedFrameOutcome r = slam.CommitTrackedFrameOnDevice(point_list, match_point, residual_norm, tOutlineThres);
    std::printf("%zu matches: %d erased, %d points went bad\n", match_point.size(), r.result.n_erased, r.result.n_bad);
    for (int32_t p : r.bad_points) std::printf("  map point %d: SetBadFlag on the caller's object\n", p);
    return r.result.n_bad;
}

// Tracking::NeedKeyframe for the same frame, on the same map: indices go up, one verdict comes back.
bool NeedKeyframeAfterTrackedFrame(DSDTM::Slam& slam, const dsdtm_camera& cam, const double* T_cur_w, const std::vector<int32_t>& cur_point, int32_t last_kf,
                                   const std::vector<int32_t>& local_kf, double min_rot, double min_trans) {
    const dsdtm_keyframe_params prm = {30, 50, 31, 0, 40.0, min_rot, min_trans};
    const dsdtm_keyframe_verdict v = slam.NeedKeyframeOnMap(cam, prm, T_cur_w, (int32_t)cur_point.size(), cur_point, last_kf, local_kf);
    std::printf("need = %d (rule %d), median displacement %.1f px over %d samples\n", v.need, v.reason, v.median_px, v.n_px);
    return v.need != 0;
}

// The gather alone on the host (a map read back): its desc() goes to need_keyframe_host of dsdtm_host.hpp. No library needed.
DSDTM::KeyframeDescHost GatherOnHost(const DSDTM::TrackMapArrays& map, const double* T_cur_w, const std::vector<int32_t>& cur_point, int32_t last_kf,
                                     const std::vector<int32_t>& local_kf) {
    return DSDTM::gather_keyframe_desc_host(map, T_cur_w, (int32_t)cur_point.size(), (int32_t)cur_point.size(), cur_point.data(), last_kf, (int32_t)local_kf.size(),
                                            local_kf.data());
}

// The same on the host, on a map read back (dsdtm_slam_map_read) or kept there: no library needed.
DSDTM::TrackCommitHost AfterTrackedFrameOnHost(const DSDTM::TrackCommitMap& map, const std::vector<int32_t>& point, const std::vector<double>& residual_norm,
                                               double tOutlineThres) {
    return DSDTM::track_commit_host(map, tOutlineThres, (int32_t)point.size(), point.data(), residual_norm.data());
}
