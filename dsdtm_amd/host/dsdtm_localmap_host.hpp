// dsdtm_localmap_host.hpp — Tracking::GetCloseKeyFrames (src/Tracking.cpp:315-345) and the keyframe and point selection of
// Tracking::UpdateLocalMap (:258-297), twice:
//
//   select_local_map_host(...)   the rules L1-L4 of include/dsdtm_amd_localmap.h on plain arrays, WITHOUT any device call or library:
//                                dependency-free C++ (this project's own straightforward loop, not the reference's code). Every
//                                product and sum rounds on its own when this header is compiled without FMA contraction
//                                (-ffp-contract=off; the x86-64 default) — then kf_dist is bit-equal to the device's.
//   DSDTM::LocalMap              a thin RAII class over the C ABI (libdsdtm_amd_localmap.so): the map resident on the device, the
//                                three updates, Select, and UpdateLocalMapOnDevice — which goes beside Tracking::TrackFrame
//                                (dsdtm_host.hpp): its `local_points` argument and mvpLocalKeyFrames from the returned indices.
//                                No CPU compute path: a failure throws.
//
// Which to call (README, profiles/r17_local_map.txt): one device select is 140-190 us whatever the map, the host function about 0.9 us per
// keyframe of 300 slots — for ONE pose per call use select_local_map_host below about 170 keyframes and LocalMap above; for 64 poses or
// more per call (dsdtm_localmap_select with n descs) the device wins from 100 keyframes on.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dsdtm_amd_localmap.h"

namespace DSDTM {

// A map as plain arrays: what dsdtm_localmap_map_read returns (keyframe k's slots are point_of_slot[slot_offset[k] .. + n_slots[k])).
struct LocalMapArrays {
    int32_t n_points = 0; const double* p_world = nullptr; const uint8_t* bad = nullptr;
    int32_t n_keyframes = 0; const double* T_kf_w = nullptr; const int32_t* n_slots = nullptr; const int64_t* slot_offset = nullptr;
    const int32_t* point_of_slot = nullptr;
};
// What a caller keeps between calls so that no call clears an array of the map's size (mLastProjectedFrameId: a stamp per point).
struct LocalMapHostScratch {
    std::vector<uint32_t> stamp;
    uint32_t frame = 0;
    std::vector<std::pair<double, int32_t>> close;
};

namespace localmap_detail {
// cvRound of a cv::Point2f member: narrowed to float first, halves to even (src/Camera.cpp:187-193)
inline int cv_round(double v) { return (int)std::nearbyint((double)(float)v); }
inline bool in_image(const dsdtm_camera& c, double x, double y, int boundary) {
    if (!(std::fabs(x) < 1e9) || !(std::fabs(y) < 1e9)) return false;
    const int xr = cv_round(x), yr = cv_round(y);
    return xr >= boundary && xr < c.width - boundary && yr >= boundary && yr < c.height - boundary;
}
// Frame::isVisible (src/Frame.cpp:300-311)
inline bool is_visible(const dsdtm_camera& c, const double* m, const double* X, int boundary) {
    const double x = m[0] * X[0] + m[1] * X[1] + m[2] * X[2] + m[3], y = m[4] * X[0] + m[5] * X[1] + m[6] * X[2] + m[7],
                 z = m[8] * X[0] + m[9] * X[1] + m[10] * X[2] + m[11];
    if (z < 0.0) return false;
    const double u = (double)c.fx * x / z + (double)c.cx, v = (double)c.fy * y / z + (double)c.cy;
    return in_image(c, u, v, boundary);
}
}  // namespace localmap_detail

// kf, kf_dist: n_local each; point, point_kf: point_capacity each. Entries from n_kf / min(n_points, point_capacity) on are left untouched.
inline void select_local_map_host(const dsdtm_camera& cam, const dsdtm_localmap_params& prm, const LocalMapArrays& m, const double* T_cur_w,
                                  int32_t* kf, double* kf_dist, int32_t point_capacity, int32_t* point, int32_t* point_kf,
                                  dsdtm_localmap_result* res, LocalMapHostScratch* scratch = nullptr) {
    LocalMapHostScratch local;
    LocalMapHostScratch& s = scratch ? *scratch : local;
    s.close.clear();
    // L1, L2 (:320-336)
    for (int32_t k = 0; k < m.n_keyframes; ++k) {
        const int32_t* sl = m.point_of_slot + m.slot_offset[k];
        for (int32_t i = 0; i < m.n_slots[k]; ++i) {
            const int32_t p = sl[i];
            if (p < 0) continue;                                                       // :324
            const double* X = m.p_world + 3 * (size_t)p;
            if (X[0] == 0.0 && X[1] == 0.0 && X[2] == 0.0) continue;                   // :327
            if (localmap_detail::is_visible(cam, T_cur_w, X, prm.boundary)) {          // :330
                const double* Tk = m.T_kf_w + 12 * (size_t)k;
                const double dx = T_cur_w[3] - Tk[3], dy = T_cur_w[7] - Tk[7], dz = T_cur_w[11] - Tk[11];
                s.close.push_back(std::make_pair(std::sqrt(dx * dx + (dy * dy + dz * dz)), k));      // :333
                break;
            }
        }
    }
    // L3 (:267-268): stable, so equal distances keep map index order
    std::stable_sort(s.close.begin(), s.close.end(),
                     [](const std::pair<double, int32_t>& a, const std::pair<double, int32_t>& b) { return a.first < b.first; });
    const int32_t n_kf = (int32_t)std::min<size_t>(s.close.size(), (size_t)prm.n_local);
    // L4 (:277-297)
    if (s.stamp.size() < (size_t)m.n_points) s.stamp.resize((size_t)m.n_points, 0u);
    if (++s.frame == 0u) { std::fill(s.stamp.begin(), s.stamp.end(), 0u); s.frame = 1u; }
    int32_t n_points = 0;
    for (int32_t j = 0; j < n_kf; ++j) {
        const int32_t k = s.close[(size_t)j].second;
        kf[j] = k; kf_dist[j] = s.close[(size_t)j].first;
        const int32_t* sl = m.point_of_slot + m.slot_offset[k];
        for (int32_t i = 0; i < m.n_slots[k]; ++i) {
            const int32_t p = sl[i];
            if (p < 0) continue;                                                       // :288
            if (m.bad[p]) continue;                                                    // :291
            if (s.stamp[(size_t)p] == s.frame) continue;                               // :294
            s.stamp[(size_t)p] = s.frame;                                              // :297
            if (n_points < point_capacity) { point[n_points] = p; point_kf[n_points] = j; }
            ++n_points;
        }
    }
    res->n_close = (int32_t)s.close.size(); res->n_kf = n_kf; res->n_points = n_points; res->overflow = n_points > point_capacity ? 1 : 0;
}

// The map of one tracker (or one rig) on the device, and the selection on it. One per calling thread (it owns a dsdtm_localmap_ctx).
class LocalMap {
public:
    struct Selection {
        std::vector<int32_t> kf; std::vector<double> kf_dist;      // n_kf: the local keyframes, nearest first
        std::vector<int32_t> point, point_kf;                      // n_points: the local points in walk order
        dsdtm_localmap_result result{};
    };

    explicit LocalMap(int device = 0) {
        if (dsdtm_localmap_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_localmap_create: ") + dsdtm_localmap_last_error(nullptr));
        if (dsdtm_localmap_map_create(ctx_, &map_) != DSDTM_OK) {
            const std::string why = dsdtm_localmap_last_error(ctx_);
            dsdtm_localmap_destroy(ctx_);
            throw std::runtime_error("dsdtm_localmap_map_create: " + why);
        }
    }
    ~LocalMap() {
        dsdtm_localmap_map_destroy(ctx_, map_);
        dsdtm_localmap_destroy(ctx_);
    }
    LocalMap(const LocalMap&) = delete;
    LocalMap& operator=(const LocalMap&) = delete;

    // Map::AddMapPoint, MapPoint::Set_Pose (after local BA), MapPoint::SetBadFlag: points [first, first + n)
    void WritePoints(int first, int n, const double* p_world, const uint8_t* bad) { check(dsdtm_localmap_points_write(ctx_, map_, first, n, p_world, bad), "dsdtm_localmap_points_write"); }
    // Map::AddKeyFrame: returns the keyframe's index
    int AddKeyFrame(const double* T_kf_w, int n_slots, const int32_t* point_of_slot) {
        int k = -1;
        check(dsdtm_localmap_keyframe_add(ctx_, map_, T_kf_w, n_slots, point_of_slot, &k), "dsdtm_localmap_keyframe_add");
        return k;
    }
    // KeyFrame::Set_Pose (T_kf_w; null: keep), KeyFrame::Add_MapPoint / Erase_MapPointMatch (slots [first_slot, first_slot + n))
    void WriteKeyFrame(int kf, const double* T_kf_w, int first_slot, int n, const int32_t* point_of_slot) {
        check(dsdtm_localmap_keyframe_write(ctx_, map_, kf, T_kf_w, first_slot, n, point_of_slot), "dsdtm_localmap_keyframe_write");
    }

    // GetCloseKeyFrames + the selection of UpdateLocalMap for the pose T_cur_w. point_capacity: at most n_local * 4096; a list that is
    // longer comes back cut (result.overflow = 1, result.n_points the full length).
    Selection Select(const dsdtm_camera& cam, const double* T_cur_w, int n_local = 10, int boundary = 0, int point_capacity = 4096) {
        Selection s;
        s.kf.resize((size_t)n_local); s.kf_dist.resize((size_t)n_local);
        s.point.resize((size_t)std::max(point_capacity, 1)); s.point_kf.resize((size_t)std::max(point_capacity, 1));
        dsdtm_localmap_params prm{n_local, boundary};
        dsdtm_localmap_desc d{};
        d.map = map_; d.T_cur_w = T_cur_w; d.kf = s.kf.data(); d.kf_dist = s.kf_dist.data();
        d.point_capacity = point_capacity; d.point = s.point.data(); d.point_kf = s.point_kf.data();
        check(dsdtm_localmap_select(ctx_, &cam, &prm, 1, &d, &s.result), "dsdtm_localmap_select");
        s.kf.resize((size_t)s.result.n_kf); s.kf_dist.resize((size_t)s.result.n_kf);
        const size_t np = (size_t)std::min(s.result.n_points, point_capacity);
        s.point.resize(np); s.point_kf.resize(np);
        return s;
    }

    // Beside Tracking::TrackFrame, from the caller's own tables (all_keyframes[i] is the object whose keyframe index is i, all_points[p]
    // the one whose point index is p — the order they were added in):
    //   local_points      TrackFrame's `local_points`: the local points in the order the reference hands them to ReprojectPoint (:299);
    //   local_keyframes   mvpLocalKeyFrames, nearest first: what NeedKeyframe takes. NOT TrackFrame's `keyframes`: a map point's
    //                     mObservations are keyed by the keyframe's index in the FULL list and Get_ClosetObs walks all of them, so
    //                     TrackFrame takes all_keyframes itself (the Python mirror, Tracker.UpdateLocalMap, returns the same).
    // A list longer than point_capacity is asked for again with room for all of it (never returned cut). Below about 170 keyframes
    // select_local_map_host on the caller's arrays is the faster call for one pose (the header's top).
    template <class KF, class MP>
    Selection UpdateLocalMapOnDevice(const dsdtm_camera& cam, const double* T_cur_w, const std::vector<KF*>& all_keyframes, const std::vector<MP*>& all_points,
                                     std::vector<KF*>* local_keyframes, std::vector<MP*>* local_points, int n_local = 10, int point_capacity = 4096) {
        Selection s = Select(cam, T_cur_w, n_local, 0, point_capacity);
        if (s.result.overflow) s = Select(cam, T_cur_w, n_local, 0, s.result.n_points);
        if (s.result.overflow) throw std::runtime_error("UpdateLocalMapOnDevice: the local point list does not fit");
        local_keyframes->clear(); local_points->clear();
        for (int32_t k : s.kf) local_keyframes->push_back(all_keyframes.at((size_t)k));
        for (int32_t p : s.point) local_points->push_back(all_points.at((size_t)p));
        return s;
    }

    dsdtm_localmap_ctx* ctx() const { return ctx_; }
    dsdtm_localmap* map() const { return map_; }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_localmap_last_error(ctx_));
    }
    dsdtm_localmap_ctx* ctx_ = nullptr;
    dsdtm_localmap* map_ = nullptr;
};

}  // namespace DSDTM
