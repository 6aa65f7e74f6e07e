// dsdtm_slam_host.hpp — dsdtm_slam_track_commit and the gather of dsdtm_slam_need_keyframes (include/dsdtm_amd_slam.h), twice:
//
//   track_commit_host
//       the same rules (T1-T3, one desc; call it desc after desc for T4) on plain arrays (a map as dsdtm_slam_map_read returns it),
//       WITHOUT any device call or library: dependency-free C++, this project's own straightforward loops over flat arrays — NOT the
//       reference's walk over std::map<KeyFrame*, ...> per MapPoint. Equal, byte for byte, to the device entry and to
//       dsdtm_amd/aftertrack_restatement.py.
//   DSDTM::Slam
//       a thin RAII class over the C ABI (libdsdtm_amd_slam.so): the ONE resident map of a process with the adapter
//       Tracking::CommitTrackedFrameOnDevice. No CPU compute path: a failure throws.
//
// Which to call (profiles/r21_aftertrack.txt, one frame of 200 matches): when no point goes bad the host function wins at every map size
// (0.2 us against 25-44 us on the device); when one goes bad it passes over every slot (1.9 / 15 / 156 / 603 us at 10 / 100 / 1000 / 4000
// keyframes of 300 slots) and the device (26-46 us) wins from about 200 keyframes on. gather_keyframe_desc_host takes 2.2 us; the device
// entry wins only in batches (0.20 us per tracker at 1024). The device entries keep the RESIDENT map true without reading it back.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_slam.h"
#include "dsdtm_trackmap_host.hpp"

namespace DSDTM {

// The map's arrays a tracked frame writes (a map as dsdtm_slam_map_read returns it; the other arrays stay as they are).
struct TrackCommitMap {
    int32_t n_points = 0;
    int32_t* found = nullptr; uint8_t* bad = nullptr;           // n_points each
    int64_t n_slots_total = 0;
    int32_t* point_of_slot = nullptr; uint8_t* observes = nullptr;      // n_slots_total each
};
struct TrackCommitHost {
    int32_t n_erased = 0;
    std::vector<int32_t> bad_points;            // map indices, in match order
    std::vector<int32_t> found_after;           // per match
};

// Rules T1-T3 for one tracked frame: IncreaseFound for every match (src/Feature_alignment.cpp:106), the EraseFound walk
// (src/Optimizer.cpp:81-94) and the SetBadFlag cascade (src/MapPoint.cpp:91-109). The caller has checked what the entry checks: every
// index inside the map, no point twice.
inline TrackCommitHost track_commit_host(const TrackCommitMap& m, double outlier_threshold, int32_t n_matches, const int32_t* point, const double* residual_norm) {
    TrackCommitHost out;
    for (int32_t i = 0; i < n_matches; ++i) m.found[point[i]] += 1;
    for (int32_t i = 0; i < n_matches; ++i) {
        const int32_t p = point[i];
        if (!(residual_norm[i] > outlier_threshold) || m.bad[p]) continue;
        m.found[p] -= 1;
        ++out.n_erased;
        if (m.found[p] <= 0) { m.bad[p] = 1; out.bad_points.push_back(p); }
    }
    out.found_after.resize((size_t)n_matches);
    for (int32_t i = 0; i < n_matches; ++i) out.found_after[(size_t)i] = m.found[point[i]];
    if (!out.bad_points.empty()) {
        std::vector<uint8_t> went_bad((size_t)m.n_points, 0);
        for (int32_t p : out.bad_points) went_bad[(size_t)p] = 1;
        for (int64_t s = 0; s < m.n_slots_total; ++s)
            if (m.observes[s] && m.point_of_slot[s] >= 0 && went_bad[(size_t)m.point_of_slot[s]]) { m.observes[s] = 0; m.point_of_slot[s] = -1; }
    }
    return out;
}

// One tracker's inputs of dsdtm_need_keyframes, gathered from a map (what dsdtm_slam_need_keyframes builds on the device).
struct KeyframeDescHost {
    double T_cur_w[12], T_kf_w[12];
    int32_t n_valid = 0;
    std::vector<double> cur_p_world, kf_p_world, local_kf_centre;
    std::vector<uint8_t> cur_bad, kf_bad;
    dsdtm_keyframe_desc desc() const {              // (valid while this object lives)
        dsdtm_keyframe_desc d;
        d.T_cur_w = T_cur_w; d.T_kf_w = T_kf_w; d.n_valid = n_valid;
        d.n_cur_points = (int32_t)cur_bad.size(); d.cur_p_world = cur_p_world.data(); d.cur_bad = cur_bad.data();
        d.n_kf_points = (int32_t)kf_bad.size(); d.kf_p_world = kf_p_world.data(); d.kf_bad = kf_bad.data();
        d.n_local_kf = (int32_t)(local_kf_centre.size() / 3); d.local_kf_centre = local_kf_centre.data();
        return d;
    }
};

// The gather: the current frame's points by map index, the last keyframe's pose and its listed slots (point_of_slot >= 0) in slot
// order, the local keyframes' camera centres c_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2). Compile with -ffp-contract=off: the sums must
// not be fused. The caller has checked the indices. Hand desc() to need_keyframe_host (dsdtm_host.hpp) or dsdtm_need_keyframes.
inline KeyframeDescHost gather_keyframe_desc_host(const TrackMapArrays& t, const double* T_cur_w, int32_t n_valid, int32_t n_cur_points, const int32_t* cur_point,
                                                  int32_t kf, int32_t n_local_kf, const int32_t* local_kf) {
    KeyframeDescHost out;
    memcpy(out.T_cur_w, T_cur_w, 96);
    memcpy(out.T_kf_w, t.sel.T_kf_w + 12 * (size_t)kf, 96);
    out.n_valid = n_valid;
    auto push = [&](std::vector<double>& p, std::vector<uint8_t>& b, int32_t i) {
        p.insert(p.end(), t.sel.p_world + 3 * (size_t)i, t.sel.p_world + 3 * (size_t)i + 3);
        b.push_back(t.sel.bad[i] ? 1 : 0);
    };
    for (int32_t i = 0; i < n_cur_points; ++i) push(out.cur_p_world, out.cur_bad, cur_point[i]);
    const int64_t off = t.sel.slot_offset[kf];
    for (int32_t s = 0; s < t.sel.n_slots[kf]; ++s)
        if (t.sel.point_of_slot[off + s] >= 0) push(out.kf_p_world, out.kf_bad, t.sel.point_of_slot[off + s]);
    for (int32_t i = 0; i < n_local_kf; ++i) {
        const double* T = t.sel.T_kf_w + 12 * (size_t)local_kf[i];
        for (int c = 0; c < 3; ++c) {
            const double a = T[c] * T[3], b = T[4 + c] * T[7], e = T[8 + c] * T[11];
            const double ab = a + b;
            out.local_kf_centre.push_back(-(ab + e));
        }
    }
    return out;
}

// The resident map of a process: tracking, mapping and the tracked frame's commit on one dsdtm_slam_ctx. One per calling thread.
class Slam {
public:
    explicit Slam(int device = 0) {
        if (dsdtm_slam_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_slam_create: ") + dsdtm_slam_last_error(nullptr));
        if (dsdtm_slam_map_create(ctx_, &map_) != DSDTM_OK) {
            const std::string why = dsdtm_slam_last_error(ctx_);
            dsdtm_slam_destroy(ctx_);
            throw std::runtime_error("dsdtm_slam_map_create: " + why);
        }
    }
    ~Slam() { dsdtm_slam_destroy(ctx_); }                   // (the map goes with its context)
    Slam(const Slam&) = delete;
    Slam& operator=(const Slam&) = delete;
    dsdtm_slam_ctx* ctx() const { return ctx_; }
    dsdtm_trackmap* map() const { return map_; }
    void Check(int status, const char* what) const {
        if (status != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_slam_last_error(ctx_));
    }

    struct TrackedFrameOutcome {
        dsdtm_slam_commit_result result{};
        std::vector<int32_t> found_after;           // per match: Get_FoundNums() of its point now
        std::vector<int32_t> bad_points;            // map indices of the points that went bad: SetBadFlag on the caller's objects
    };
    // Tracking::CommitTrackedFrameOnDevice: what TrackWithLocalMap leaves on the map (src/Tracking.cpp:219-256), on the resident map.
    // point_list: the `point` column dsdtm_slam_local returned for this frame; match_point[k]: ms[k].point of dsdtm_track_frame(s)
    // (an index into that list); residual_norm: its norms; outlier_threshold: tOutlineThres (src/Optimizer.cpp:22-24). A lost frame
    // passes no matches.
    TrackedFrameOutcome CommitTrackedFrameOnDevice(const std::vector<int32_t>& point_list, const std::vector<int32_t>& match_point,
                                                   const std::vector<double>& residual_norm, double outlier_threshold) {
        if (match_point.size() != residual_norm.size()) throw std::invalid_argument("CommitTrackedFrameOnDevice: one norm per match");
        std::vector<int32_t> point(match_point.size());
        for (size_t k = 0; k < match_point.size(); ++k) point[k] = point_list.at((size_t)match_point[k]);
        TrackedFrameOutcome out;
        const int32_t n = (int32_t)point.size();
        out.found_after.resize(point.size());
        out.bad_points.resize(point.size());
        dsdtm_slam_commit_desc d = {map_, n, 0, point.data(), residual_norm.data(), out.found_after.data()};
        Check(dsdtm_slam_track_commit(ctx_, outlier_threshold, 1, &d, n, out.bad_points.data(), &out.result), "dsdtm_slam_track_commit");
        out.bad_points.resize((size_t)out.result.n_bad);
        return out;
    }

    // Tracking::NeedKeyframeOnMap: NeedKeyframe() (src/Tracking.cpp:347-410) for the tracked frame on the resident map. cur_point: the
    // frame's map points as map indices in feature order; kf: the last keyframe's map index; local_kf: mvpLocalKeyFrames as map indices.
    dsdtm_keyframe_verdict NeedKeyframeOnMap(const dsdtm_camera& cam, const dsdtm_keyframe_params& params, const double* T_cur_w, int32_t n_valid,
                                             const std::vector<int32_t>& cur_point, int32_t kf, const std::vector<int32_t>& local_kf) {
        dsdtm_slam_keyframe_desc d = {map_, T_cur_w, n_valid, (int32_t)cur_point.size(), cur_point.data(), kf, (int32_t)local_kf.size(), local_kf.data()};
        dsdtm_keyframe_verdict v{};
        Check(dsdtm_slam_need_keyframes(ctx_, &cam, &params, 1, &d, &v), "dsdtm_slam_need_keyframes");
        return v;
    }

private:
    dsdtm_slam_ctx* ctx_ = nullptr;
    dsdtm_trackmap* map_ = nullptr;
};

}  // namespace DSDTM
