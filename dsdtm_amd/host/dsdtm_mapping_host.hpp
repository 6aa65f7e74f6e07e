// dsdtm_mapping_host.hpp — the three entries of include/dsdtm_amd_mapping.h, twice:
//
//   update_connection_host / ba_window_host / ba_commit_host
//       the same rules on plain arrays (a map as dsdtm_mapping_map_read returns it), WITHOUT any device call or library: dependency-free
//       C++, this project's own straightforward loops over flat arrays — NOT the reference's walk over std::map<KeyFrame*, ...> per
//       MapPoint. Integers equal and doubles bit-equal to the device entries and to dsdtm_amd/ba_window_restatement.py (every value is
//       a copy).
//   DSDTM::Mapping
//       a thin RAII class over the C ABI (libdsdtm_amd_mapping.so): the map resident on the device with its updates, and the adapters
//       KeyFrame::UpdateConnectionOnDevice and Optimizer::LocalBundleAdjustmentOnDevice (window -> dsdtm_local_ba_batch_device ->
//       commit). Device memory is the caller's. No CPU compute path: a failure throws.
//
// Which to call (profiles/r19_ba_window.txt): for ONE keyframe per call update_connection_host wins below about 600 keyframes and
// ba_window_host below about 1000 (18 / 30 / 214 / 862 us against 116 / 182 / 223 / 391 us on the device at 10 / 100 / 1000 / 4000 keyframes of
// 300 slots); from 16 windows per call the device wins at every size. The device path keeps the map resident; the step is the solve's.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dsdtm_amd_mapping.h"
#include "dsdtm_trackmap_host.hpp"

namespace DSDTM {

struct CovisibilityHost {
    std::vector<int32_t> cov_kf, cov_weight;    // the whole sorted list: ascending (weight, keyframe index)
    int32_t n_connected = 0;                    // keyframes with weight > 0 (mConnectedKFs)
};

// KeyFrame::UpdateConnection (src/Keyframe.cpp:71-133): the rules of dsdtm_mapping_covisibility.
inline CovisibilityHost update_connection_host(const TrackMapArrays& t, int32_t kf) {
    const LocalMapArrays& a = t.sel;
    std::vector<int32_t> mult((size_t)a.n_points, 0), weight((size_t)a.n_keyframes, 0);
    for (int32_t s = 0; s < a.n_slots[kf]; ++s) {           // mvMapPoints is walked: the slot's own `observes` is not consulted
        const int32_t p = a.point_of_slot[a.slot_offset[kf] + s];
        if (p >= 0 && !a.bad[p]) ++mult[(size_t)p];
    }
    for (int32_t k = 0; k < a.n_keyframes; ++k) {
        if (k == kf) continue;
        for (int32_t s = 0; s < a.n_slots[k]; ++s) {
            const int64_t at = a.slot_offset[k] + s;
            if (t.observes[at] && a.point_of_slot[at] >= 0) weight[(size_t)k] += mult[(size_t)a.point_of_slot[at]];
        }
    }
    CovisibilityHost out;
    std::vector<std::pair<int32_t, int32_t>> pairs;
    int32_t best_w = 0, best_k = -1;
    for (int32_t k = 0; k < a.n_keyframes; ++k) {
        const int32_t w = weight[(size_t)k];
        if (w <= 0) continue;
        ++out.n_connected;
        if (w > best_w) { best_w = w; best_k = k; }          // strict: the lowest index wins among equals
        if (w > DSDTM_MAPPING_COV_THRESHOLD) pairs.emplace_back(w, k);
    }
    if (pairs.empty() && best_k >= 0) pairs.emplace_back(best_w, best_k);
    std::sort(pairs.begin(), pairs.end());
    for (const auto& p : pairs) { out.cov_weight.push_back(p.first); out.cov_kf.push_back(p.second); }
    return out;
}

// One window as dsdtm_mapping_ba_window builds it; the columns are filled only when result.usable.
struct BaWindowHost {
    dsdtm_mapping_window_result result{};
    std::vector<int32_t> kf_index, point_index, obs_kf, obs_point, obs_level;
    std::vector<int64_t> obs_slot;
    std::vector<uint8_t> kf_constant;
    std::vector<double> T_c2w, points, obs_bearing;
};

// Optimizer::LocalBundleAdjustment's sets and blocks (src/Optimizer.cpp:109-159, :166-224): rules W1-W4. The caller has checked cov_kf
// (no kf, no repeat, indices of the map), as the device entry does.
inline BaWindowHost ba_window_host(const TrackMapArrays& t, int32_t kf, int32_t n_cov, const int32_t* cov_kf, int32_t origin_kf, int32_t keyframe_capacity,
                                   int32_t point_capacity, int32_t observation_capacity) {
    const LocalMapArrays& a = t.sel;
    BaWindowHost w;
    std::vector<int32_t> local(1, kf);
    local.insert(local.end(), cov_kf, cov_kf + n_cov);
    std::vector<int32_t> kfwin((size_t)a.n_keyframes, -1), lp_of((size_t)a.n_points, -1), points;
    for (size_t r = 0; r < local.size(); ++r) kfwin[(size_t)local[r]] = (int32_t)r;
    if (kf != origin_kf)                                    // the quirk of :135: a window whose keyframe is the origin collects no points
        for (int32_t k : local)
            for (int32_t s = 0; s < a.n_slots[k]; ++s) {
                const int32_t p = a.point_of_slot[a.slot_offset[k] + s];
                if (p < 0 || a.bad[p] || lp_of[(size_t)p] >= 0) continue;
                lp_of[(size_t)p] = (int32_t)points.size();
                points.push_back(p);
            }
    // every observing slot of a window point, keyed (window point, keyframe, slot): sorted, that is W4's order, and W3's first occurrences
    struct Obs { int32_t lp, k, s; };
    std::vector<Obs> obs;
    for (int32_t k = 0; k < a.n_keyframes; ++k)
        for (int32_t s = 0; s < a.n_slots[k]; ++s) {
            const int64_t at = a.slot_offset[k] + s;
            const int32_t p = t.observes[at] ? a.point_of_slot[at] : -1;
            if (p >= 0 && lp_of[(size_t)p] >= 0) obs.push_back({lp_of[(size_t)p], k, s});
        }
    std::stable_sort(obs.begin(), obs.end(), [](const Obs& x, const Obs& y) { return x.lp < y.lp; });      // (keyframe, slot) ascend already
    std::vector<int32_t> fixed;
    for (const Obs& o : obs)
        if (kfwin[(size_t)o.k] < 0) { kfwin[(size_t)o.k] = (int32_t)(local.size() + fixed.size()); fixed.push_back(o.k); }
    int32_t origin_local = 0;
    for (int32_t k : local) origin_local |= k == origin_kf ? 1 : 0;
    dsdtm_mapping_window_result& r = w.result;
    r.n_local = (int32_t)local.size(); r.n_fixed = (int32_t)fixed.size(); r.n_points = (int32_t)points.size(); r.n_obs = (int32_t)obs.size();
    const int32_t n_free = r.n_local - origin_local;
    r.over_free_kf = n_free > DSDTM_LBA_MAX_FREE_KF; r.over_const_kf = r.n_fixed + origin_local > DSDTM_LBA_MAX_CONST_KF;
    r.over_points = r.n_points > DSDTM_LBA_MAX_POINTS; r.over_obs = r.n_obs > DSDTM_LBA_MAX_OBSERVATIONS;
    r.over_keyframe_capacity = r.n_local + r.n_fixed > keyframe_capacity; r.over_point_capacity = r.n_points > point_capacity;
    r.over_observation_capacity = r.n_obs > observation_capacity;
    r.usable = n_free >= 1 && !(r.over_free_kf | r.over_const_kf | r.over_points | r.over_obs | r.over_keyframe_capacity | r.over_point_capacity |
                                r.over_observation_capacity);
    if (!r.usable) return w;
    w.kf_index = local;
    w.kf_index.insert(w.kf_index.end(), fixed.begin(), fixed.end());
    for (size_t i = 0; i < w.kf_index.size(); ++i) {
        const int32_t k = w.kf_index[i];
        w.kf_constant.push_back(i >= local.size() || k == origin_kf ? 1 : 0);
        w.T_c2w.insert(w.T_c2w.end(), a.T_kf_w + 12 * (size_t)k, a.T_kf_w + 12 * (size_t)k + 12);
    }
    w.point_index = points;
    for (int32_t p : points) w.points.insert(w.points.end(), a.p_world + 3 * (size_t)p, a.p_world + 3 * (size_t)p + 3);
    for (const Obs& o : obs) {
        const int64_t at = a.slot_offset[o.k] + o.s;
        w.obs_kf.push_back(kfwin[(size_t)o.k]); w.obs_point.push_back(o.lp); w.obs_level.push_back(t.level[at]);
        w.obs_slot.push_back((int64_t)(((uint64_t)(uint32_t)o.k << 32) | (uint32_t)o.s));
        w.obs_bearing.insert(w.obs_bearing.end(), t.bearing + 3 * (size_t)at, t.bearing + 3 * (size_t)at + 3);
    }
    return w;
}

// The map's arrays the commit writes (the others of a TrackMapArrays stay as they are).
struct MappingMapWritable {
    double* p_world; uint8_t* bad; double* T_kf_w; const int64_t* slot_offset; int32_t* point_of_slot; uint8_t* observes;
};
struct BaCommitHost {
    int32_t n_outliers = 0;
    std::vector<int32_t> bad_points;            // map indices, in window point order
};

// The write-back and the outlier pass (src/Optimizer.cpp:236-271, src/MapPoint.cpp:57-109): rules C1, C2 for one usable window whose
// T_c2w / points hold the solver's output.
inline BaCommitHost ba_commit_host(const MappingMapWritable& m, const BaWindowHost& w, const double* T_c2w, const double* points, const uint8_t* outlier) {
    BaCommitHost out;
    for (size_t i = 0; i < w.kf_index.size(); ++i) memcpy(m.T_kf_w + 12 * (size_t)w.kf_index[i], T_c2w + 12 * i, 96);
    for (size_t i = 0; i < w.point_index.size(); ++i) memcpy(m.p_world + 3 * (size_t)w.point_index[i], points + 3 * i, 24);
    size_t j0 = 0;
    for (size_t i = 0; i < w.point_index.size(); ++i) {
        size_t j1 = j0;
        while (j1 < w.obs_point.size() && w.obs_point[j1] == (int32_t)i) ++j1;
        const int32_t n0 = (int32_t)(j1 - j0);
        int32_t erased = 0;
        bool bad = false;
        for (size_t j = j0; j < j1; ++j) {
            if (!outlier[j]) continue;
            ++out.n_outliers;
            if (bad) continue;                              // (Erase_Observation finds nothing: the observations are gone)
            ++erased;
            if (n0 - erased <= 1) bad = true;
        }
        int32_t seen = 0;
        for (size_t j = j0; j < j1; ++j) {
            const uint64_t key = (uint64_t)w.obs_slot[j];
            const int64_t at = m.slot_offset[(size_t)(key >> 32)] + (int64_t)(key & 0xffffffffu);
            if (outlier[j] && seen < erased) { ++seen; m.observes[at] = 0; }        // the slot is KEPT
            else if (bad) { m.observes[at] = 0; m.point_of_slot[at] = -1; }        // SetBadFlag: what is still left
        }
        if (bad) { m.bad[w.point_index[i]] = 1; out.bad_points.push_back(w.point_index[i]); }
        j0 = j1;
    }
    return out;
}

// The resident map as the mapping thread holds it. One per calling thread (it owns a dsdtm_mapping_ctx).
class Mapping {
public:
    explicit Mapping(int device = 0) {
        if (dsdtm_mapping_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_mapping_create: ") + dsdtm_mapping_last_error(nullptr));
        if (dsdtm_mapping_map_create(ctx_, &map_) != DSDTM_OK) {
            const std::string why = dsdtm_mapping_last_error(ctx_);
            dsdtm_mapping_destroy(ctx_);
            throw std::runtime_error("dsdtm_mapping_map_create: " + why);
        }
    }
    ~Mapping() { dsdtm_mapping_destroy(ctx_); }             // (the map goes with its context)
    Mapping(const Mapping&) = delete;
    Mapping& operator=(const Mapping&) = delete;
    dsdtm_mapping_ctx* ctx() const { return ctx_; }
    dsdtm_trackmap* map() const { return map_; }
    void Check(int status, const char* what) const {
        if (status != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_mapping_last_error(ctx_));
    }

    // KeyFrame::UpdateConnectionOnDevice: mOrderedCovGraph of keyframe `kf` as (weight, keyframe index) pairs, ascending. An empty list
    // with n_connected == 0 means "leave mOrderedCovGraph as it was" (:98-99).
    std::vector<std::pair<int32_t, int32_t>> UpdateConnectionOnDevice(int32_t kf, int32_t* n_connected = nullptr, int32_t capacity = 256) {
        for (;;) {
            std::vector<int32_t> k((size_t)capacity), w((size_t)capacity);
            dsdtm_mapping_cov_desc d = {map_, kf, capacity, k.data(), w.data()};
            dsdtm_mapping_cov_result r{};
            Check(dsdtm_mapping_covisibility(ctx_, 1, &d, &r), "dsdtm_mapping_covisibility");
            if (r.overflow) { capacity = r.n_cov; continue; }
            if (n_connected) *n_connected = r.n_connected;
            std::vector<std::pair<int32_t, int32_t>> out;
            for (int32_t i = 0; i < r.n_cov; ++i) out.emplace_back(w[(size_t)i], k[(size_t)i]);
            return out;
        }
    }

    struct LocalBaOutcome {
        bool usable = false;                        // false: take the host path for this keyframe
        dsdtm_mapping_window_result window{};
        dsdtm_local_ba_problem problem{};
        dsdtm_mapping_commit_result commit{};
        std::vector<int32_t> bad_points;            // map indices of the points that went bad
    };
    // Optimizer::LocalBundleAdjustmentOnDevice: window -> dsdtm_local_ba_batch_device -> commit for keyframe `kf` with its stored
    // GetCovKFrames() (map indices, in its order). `arrays`, `d_outlier` (observation_capacity bytes) and `d_summary` (one
    // dsdtm_local_ba_summary) are the caller's DEVICE memory, sized by the capacities; `solver` is the caller's dsdtm_ctx; the solve is
    // enqueued on hip_stream and the commit orders itself behind it. The host mirrors the bookkeeping on its objects from
    // arrays.h_kf_index / h_point_index / h_obs_slot, the outlier flags and bad_points.
    LocalBaOutcome LocalBundleAdjustmentOnDevice(dsdtm_ctx* solver, int32_t kf, const std::vector<int32_t>& cov_kf, int32_t origin_kf,
                                                 const dsdtm_local_ba_params& params, const dsdtm_mapping_window_arrays& arrays, int32_t keyframe_capacity,
                                                 int32_t point_capacity, int32_t observation_capacity, uint8_t* d_outlier, dsdtm_local_ba_summary* d_summary,
                                                 void* hip_stream, int32_t bad_capacity = 256) {
        LocalBaOutcome out;
        dsdtm_mapping_window_desc d = {map_, kf, (int32_t)cov_kf.size(), cov_kf.data(), origin_kf, keyframe_capacity, point_capacity, observation_capacity};
        Check(dsdtm_mapping_ba_window(ctx_, 1, &d, &arrays, &out.problem, &out.window), "dsdtm_mapping_ba_window");
        out.usable = out.window.usable != 0;
        if (!out.usable) return out;
        if (dsdtm_local_ba_batch_device(solver, 1, &out.problem, arrays.T_c2w, arrays.kf_constant, arrays.points, arrays.obs_kf, arrays.obs_point,
                                        arrays.obs_bearing, arrays.obs_level, &params, d_outlier, d_summary, hip_stream) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_local_ba_batch_device: ") + dsdtm_last_error(solver));
        out.bad_points.resize((size_t)std::max(bad_capacity, 1));
        Check(dsdtm_mapping_ba_commit(ctx_, 1, &d, &out.problem, &out.window, &arrays, d_outlier, hip_stream, bad_capacity, out.bad_points.data(), &out.commit),
              "dsdtm_mapping_ba_commit");
        out.bad_points.resize((size_t)std::min(out.commit.n_bad, bad_capacity));
        return out;
    }

private:
    dsdtm_mapping_ctx* ctx_ = nullptr;
    dsdtm_trackmap* map_ = nullptr;
};

}  // namespace DSDTM
