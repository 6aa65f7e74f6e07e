// dsdtm_trackmap_host.hpp — dsdtm_track_desc's local-map columns (include/dsdtm_amd.h: mp_world .. obs_bearing) for the points the
// selection of Tracking::UpdateLocalMap emits, twice:
//
//   flatten_local_map_host(...)   the flatten of include/dsdtm_amd_trackmap.h on plain arrays, WITHOUT any device call or library:
//                                 dependency-free C++ (this project's own straightforward loops over flat arrays — NOT the reference's
//                                 walk over std::map<KeyFrame*, ...> per MapPoint, which chases pointers and would be slower). With
//                                 select_local_map_host (dsdtm_localmap_host.hpp) in front of it, it is the whole of dsdtm_trackmap_local.
//   DSDTM::TrackMap               a thin RAII class over the C ABI (libdsdtm_amd_trackmap.so): the map resident on the device, the
//                                 updates, Local, and UpdateLocalMapOnDevice, whose columns go into a dsdtm_track_desc as they are.
//                                 No CPU compute path: a failure throws.
//
// Which to call (README, INTEGRATION §5j, profiles/r18_track_map.txt; ~2400 local points): one device call for one pose is 203-314 us whatever
// the map, select_local_map_host + flatten_local_map_host 16 / 136 / 1148 / 3988 us at 10 / 100 / 1000 / 4000 keyframes of 300 slots — for ONE
// pose use the host functions below a few hundred keyframes (the crossover lies near 220) and TrackMap above; for 64 poses or more per
// call (dsdtm_trackmap_local with n descs, capacities that fit) the device wins at every measured size.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_trackmap.h"
#include "dsdtm_localmap_host.hpp"

namespace DSDTM {

// A track map as plain arrays: what dsdtm_trackmap_map_read returns. The selection reads its LocalMapArrays part.
struct TrackMapArrays {
    LocalMapArrays sel;                 // points, bad flags, keyframe poses, slot counts and offsets, point_of_slot
    const int32_t* found = nullptr;     // per point
    const uint8_t* observes = nullptr;  // per slot of the pool, like point_of_slot
    const float* px_xy = nullptr; const int32_t* level = nullptr; const double* bearing = nullptr;      // per slot: x 2, x 1, x 3
};
// What a caller keeps between calls so that no call clears an array of the map's size
struct TrackMapHostScratch {
    std::vector<int32_t> pos;           // per map point: its position among the emitted points, -1 otherwise
    std::vector<int32_t> cursor;
};

// The columns for the m emitted points point[0 .. m) (distinct map indices: what select_local_map_host wrote, m = min(n_points,
// point_capacity)). Point i's observations are the observing slots of ALL keyframes that name it, in ascending (keyframe, slot)
// order. obs_offset[0 .. m] is the full prefix sum and *n_obs its end; only observations j < obs_capacity are written.
inline void flatten_local_map_host(const TrackMapArrays& t, int32_t m, const int32_t* point, int32_t obs_capacity, double* mp_world, int32_t* mp_found,
                                   uint8_t* mp_bad, int32_t* obs_offset, int32_t* obs_kf, float* obs_px, int32_t* obs_level, double* obs_bearing,
                                   int32_t* n_obs, TrackMapHostScratch* scratch = nullptr) {
    TrackMapHostScratch local;
    TrackMapHostScratch& s = scratch ? *scratch : local;
    const LocalMapArrays& a = t.sel;
    if (s.pos.size() < (size_t)a.n_points) s.pos.resize((size_t)a.n_points, -1);
    s.cursor.assign((size_t)m + 1, 0);
    for (int32_t i = 0; i < m; ++i) {
        const int32_t p = point[i];
        s.pos[(size_t)p] = i;
        memcpy(mp_world + 3 * (size_t)i, a.p_world + 3 * (size_t)p, 24);
        mp_found[i] = t.found[p];
        mp_bad[i] = a.bad[p] ? 1 : 0;
    }
    // count, prefix sum, fill: the second pass meets a point's observations in (keyframe, slot) order already
    for (int pass = 0; pass < 2; ++pass) {
        for (int32_t k = 0; k < a.n_keyframes; ++k) {
            const int64_t base = a.slot_offset[k];
            for (int32_t sl = 0; sl < a.n_slots[k]; ++sl) {
                if (!t.observes[base + sl]) continue;
                const int32_t p = a.point_of_slot[base + sl];
                const int32_t i = p >= 0 ? s.pos[(size_t)p] : -1;
                if (i < 0) continue;
                if (pass == 0) { ++s.cursor[(size_t)i]; continue; }
                const int32_t j = obs_offset[i] + s.cursor[(size_t)i]++;
                if (j >= obs_capacity) continue;
                obs_kf[j] = k;
                obs_px[2 * (size_t)j] = t.px_xy[2 * (size_t)(base + sl)]; obs_px[2 * (size_t)j + 1] = t.px_xy[2 * (size_t)(base + sl) + 1];
                obs_level[j] = t.level[base + sl];
                memcpy(obs_bearing + 3 * (size_t)j, t.bearing + 3 * (size_t)(base + sl), 24);
            }
        }
        if (pass == 0) {
            int32_t sum = 0;
            for (int32_t i = 0; i < m; ++i) { obs_offset[i] = sum; sum += s.cursor[(size_t)i]; s.cursor[(size_t)i] = 0; }
            obs_offset[m] = sum;
            *n_obs = sum;
        }
    }
    for (int32_t i = 0; i < m; ++i) s.pos[(size_t)point[i]] = -1;
}

// The track map of one tracker (or one rig) on the device. One per calling thread (it owns a dsdtm_trackmap_ctx).
class TrackMap {
public:
    // What a dsdtm_track_desc takes: n_points = point.size(), mp_world = this->mp_world.data(), ... (FillDesc does it)
    struct Columns {
        std::vector<int32_t> kf; std::vector<double> kf_dist;      // n_kf: the local keyframes, nearest first (what NeedKeyframe takes)
        std::vector<int32_t> point, point_kf;                      // the local points in ReprojectPoint order
        std::vector<double> mp_world; std::vector<int32_t> mp_found; std::vector<uint8_t> mp_bad; std::vector<int32_t> obs_offset;
        std::vector<int32_t> obs_kf; std::vector<float> obs_px; std::vector<int32_t> obs_level; std::vector<double> obs_bearing;
        dsdtm_trackmap_result result{};
        // The local-map columns of `d`. d->kf and d->T_kf_w stay the caller's: EVERY keyframe of the map in index order (obs_kf
        // indexes that list).
        void FillDesc(dsdtm_track_desc* d) const {
            d->n_points = (int32_t)point.size();
            d->mp_world = mp_world.data(); d->mp_found = mp_found.data(); d->mp_bad = mp_bad.data(); d->obs_offset = obs_offset.data();
            d->obs_kf = obs_kf.data(); d->obs_px = obs_px.data(); d->obs_level = obs_level.data(); d->obs_bearing = obs_bearing.data();
        }
    };

    explicit TrackMap(int device = 0) {
        if (dsdtm_trackmap_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_trackmap_create: ") + dsdtm_trackmap_last_error(nullptr));
        if (dsdtm_trackmap_map_create(ctx_, &map_) != DSDTM_OK) {
            const std::string why = dsdtm_trackmap_last_error(ctx_);
            dsdtm_trackmap_destroy(ctx_);
            throw std::runtime_error("dsdtm_trackmap_map_create: " + why);
        }
    }
    ~TrackMap() {
        dsdtm_trackmap_map_destroy(ctx_, map_);
        dsdtm_trackmap_destroy(ctx_);
    }
    TrackMap(const TrackMap&) = delete;
    TrackMap& operator=(const TrackMap&) = delete;

    // Map::AddMapPoint, MapPoint::Set_Pose (after local BA), SetBadFlag: points [first, first + n); bad / found may be null
    void WritePoints(int first, int n, const double* p_world, const uint8_t* bad, const int32_t* found) {
        check(dsdtm_trackmap_points_write(ctx_, map_, first, n, p_world, bad, found), "dsdtm_trackmap_points_write");
    }
    // MapPoint::IncreaseFound / EraseFound of a tracked frame's matches
    void WriteFound(int n, const int32_t* index, const int32_t* found) { check(dsdtm_trackmap_found_write(ctx_, map_, n, index, found), "dsdtm_trackmap_found_write"); }
    // Tracking::CraeteKeyframe: returns the keyframe's index
    int AddKeyFrame(const double* T_kf_w, int n_slots, const int32_t* point_of_slot, const uint8_t* observes, const float* px_xy, const int32_t* level,
                    const double* bearing) {
        int k = -1;
        check(dsdtm_trackmap_keyframe_add(ctx_, map_, T_kf_w, n_slots, point_of_slot, observes, px_xy, level, bearing, &k), "dsdtm_trackmap_keyframe_add");
        return k;
    }
    // KeyFrame::Set_Pose (T_kf_w; null: keep), Add_MapPoint / Add_Observation, Erase_MapPointMatch, Erase_Observation
    void WriteKeyFrame(int kf, const double* T_kf_w, int first_slot, int n, const int32_t* point_of_slot, const uint8_t* observes) {
        check(dsdtm_trackmap_keyframe_write(ctx_, map_, kf, T_kf_w, first_slot, n, point_of_slot, observes), "dsdtm_trackmap_keyframe_write");
    }

    // dsdtm_trackmap_local for one pose into *c, whose vectors are reused from call to call (a caller keeps one Columns per tracker: no
    // allocation once they have grown); the columns come back cut to what was written (result has the flags and full counts). The
    // read-back is sized by the capacities: pass capacities near the need.
    void Local(const dsdtm_camera& cam, const double* T_cur_w, Columns* c, int n_local, int boundary, int point_capacity, int obs_capacity) {
        const size_t P = (size_t)std::max(point_capacity, 1), O = (size_t)std::max(obs_capacity, 1);
        c->kf.resize((size_t)n_local); c->kf_dist.resize((size_t)n_local);
        c->point.resize(P); c->point_kf.resize(P); c->mp_world.resize(3 * P); c->mp_found.resize(P); c->mp_bad.resize(P); c->obs_offset.resize(P + 1);
        c->obs_kf.resize(O); c->obs_px.resize(2 * O); c->obs_level.resize(O); c->obs_bearing.resize(3 * O);
        dsdtm_localmap_params prm{n_local, boundary};
        dsdtm_trackmap_desc d{};
        d.map = map_; d.T_cur_w = T_cur_w; d.point_capacity = point_capacity; d.obs_capacity = obs_capacity;
        d.kf = c->kf.data(); d.kf_dist = c->kf_dist.data(); d.point = c->point.data(); d.point_kf = c->point_kf.data();
        d.mp_world = c->mp_world.data(); d.mp_found = c->mp_found.data(); d.mp_bad = c->mp_bad.data(); d.obs_offset = c->obs_offset.data();
        d.obs_kf = c->obs_kf.data(); d.obs_px = c->obs_px.data(); d.obs_level = c->obs_level.data(); d.obs_bearing = c->obs_bearing.data();
        check(dsdtm_trackmap_local(ctx_, &cam, &prm, 1, &d, &c->result), "dsdtm_trackmap_local");
        const size_t m = (size_t)std::min(c->result.n_points, point_capacity), o = (size_t)std::min(c->result.n_obs, obs_capacity);
        c->kf.resize((size_t)c->result.n_kf); c->kf_dist.resize((size_t)c->result.n_kf);
        c->point.resize(m); c->point_kf.resize(m); c->mp_world.resize(3 * m); c->mp_found.resize(m); c->mp_bad.resize(m); c->obs_offset.resize(m + 1);
        c->obs_kf.resize(o); c->obs_px.resize(2 * o); c->obs_level.resize(o); c->obs_bearing.resize(3 * o);
    }

    // Beside Tracking::TrackFrame: the finished columns for the pose T_cur_w in *desc_columns (kept by the caller from frame to frame),
    // ready for Columns::FillDesc. The capacities are REMEMBERED: what the last call needed plus a quarter and 256 (the first call:
    // 4096 points, 8192 observations), because the read-back is sized by them — with capacities near the need a call is the 203-314 us
    // of the header's top; the limits (4096 points with 16 observations each) would read back 2.8 MB per call, which was not measured.
    // obs_capacity > 0 overrides the remembered one. A list that does not fit is asked for again with room for all of it; more local
    // points than dsdtm_track_desc takes (4096) throw — never a cut result. For ONE pose on a small map select_local_map_host +
    // flatten_local_map_host on the caller's own arrays is the faster call (the header's top).
    void UpdateLocalMapOnDevice(const dsdtm_camera& cam, const double* T_cur_w, Columns* desc_columns, int n_local = 10, int obs_capacity = 0) {
        Columns* c = desc_columns;
        int pcap = point_hint_, ocap = obs_capacity > 0 ? obs_capacity : obs_hint_;
        Local(cam, T_cur_w, c, n_local, 0, pcap, ocap);
        if (c->result.overflow_points || c->result.overflow_obs) {
            if (c->result.overflow_points) pcap = DSDTM_TRACKMAP_MAX_LOCAL_POINTS;
            if (c->result.overflow_obs || c->result.overflow_points) ocap = std::max(ocap, c->result.overflow_points ? 2 * c->result.n_obs + 256 : c->result.n_obs);
            Local(cam, T_cur_w, c, n_local, 0, pcap, ocap);
            if (c->result.overflow_obs && !c->result.overflow_points) Local(cam, T_cur_w, c, n_local, 0, pcap, c->result.n_obs);
        }
        if (c->result.overflow_points || c->result.overflow_obs) throw std::runtime_error("UpdateLocalMapOnDevice: the local map does not fit a dsdtm_track_desc");
        point_hint_ = std::min(DSDTM_TRACKMAP_MAX_LOCAL_POINTS, c->result.n_points + c->result.n_points / 4 + 256);
        obs_hint_ = c->result.n_obs + c->result.n_obs / 4 + 256;
    }

    dsdtm_trackmap_ctx* ctx() const { return ctx_; }
    dsdtm_trackmap* map() const { return map_; }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_trackmap_last_error(ctx_));
    }
    dsdtm_trackmap_ctx* ctx_ = nullptr;
    dsdtm_trackmap* map_ = nullptr;
    int point_hint_ = DSDTM_TRACKMAP_MAX_LOCAL_POINTS, obs_hint_ = 8192;      // UpdateLocalMapOnDevice's remembered capacities
};

}  // namespace DSDTM
