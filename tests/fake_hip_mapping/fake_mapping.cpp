// Fakes of the launch functions of dsdtm_amd/csrc/mapping.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified and
// knows nothing of them (the map's own launches are the fakes of tests/fake_hip_trackmap and tests/fake_hip_localmap). That runtime runs
// queued operations only when something waits for them, so each fake first drains the stream. Each fake turns the device arrays of a
// record into plain arrays and answers with the host functions of dsdtm_amd/host/dsdtm_mapping_host.hpp through the block's offsets, and
// writes over the whole room of every temporary — under AddressSanitizer an offset, a count or a stale pointer that leaves its
// allocation shows up here. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_mapping.h"
#include "mapping.h"
#include "../../dsdtm_amd/host/dsdtm_mapping_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_mapping_fail(long nth) { g_fail = nth; }
long fake_mapping_launches() { return g_launches; }

static bool enter(hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return false;
    ++g_launches;
    return hipStreamSynchronize(stream) == hipSuccess;
}

namespace {

// a map's device arrays as the host functions take them
struct HostMap {
    std::vector<double> p, T, bearing;
    std::vector<uint8_t> bad, observes;
    std::vector<int32_t> ns, slots, level, found;
    std::vector<int64_t> off;
    std::vector<float> px;
    DSDTM::TrackMapArrays t;
    HostMap(const dsdtm::LmPointDev* points, const dsdtm::LmKeyframeDev* kfs, const int32_t* d_slots, const int32_t* obs, const dsdtm::TmFeatDev* feat, int K, int P)
        : p(3 * (size_t)P), T(12 * (size_t)K), bad((size_t)P), ns((size_t)K), found((size_t)P, 0), off((size_t)K) {
        size_t S = 0;
        for (int i = 0; i < P; ++i) { p[3 * (size_t)i] = points[i].x; p[3 * (size_t)i + 1] = points[i].y; p[3 * (size_t)i + 2] = points[i].z; bad[(size_t)i] = points[i].bad ? 1 : 0; }
        for (int k = 0; k < K; ++k) {
            memcpy(&T[12 * (size_t)k], kfs[k].T, 96); ns[(size_t)k] = kfs[k].n_slots; off[(size_t)k] = kfs[k].slot_off;
            S = std::max(S, (size_t)(kfs[k].slot_off + kfs[k].n_slots));
        }
        slots.assign(d_slots, d_slots + S);
        observes.resize(S); level.resize(S); px.resize(2 * S); bearing.resize(3 * S);
        for (size_t s = 0; s < S; ++s) {
            observes[s] = obs[s] >= 0 ? 1 : 0;
            if (feat) { level[s] = feat[s].level; memcpy(&bearing[3 * s], feat[s].bearing, 24); }
        }
        t.sel.n_points = P; t.sel.p_world = p.data(); t.sel.bad = bad.data(); t.sel.n_keyframes = K; t.sel.T_kf_w = T.data(); t.sel.n_slots = ns.data();
        t.sel.slot_offset = off.data(); t.sel.point_of_slot = slots.data();
        t.found = found.data(); t.observes = observes.data(); t.px_xy = px.data(); t.level = level.data(); t.bearing = bearing.data();
    }
};

}  // namespace

namespace dsdtm {

hipError_t mapping_covisibility_launch(const MpCovArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (((size_t)a.block) & 7)) return hipErrorInvalidValue;
    for (int t = 0; t < a.n; ++t) {
        MpCovDev d;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        if (d.K > a.max_K) return hipErrorInvalidValue;
        int P = 0;
        for (int k = 0; k < d.K; ++k)
            for (int s = 0; s < d.kfs[k].n_slots; ++s) P = std::max(P, d.slots[d.kfs[k].slot_off + s] + 1);
        HostMap m(d.points, d.kfs, d.slots, d.obs, nullptr, d.K, P);
        memset(a.block + d.weight, 0, (size_t)d.K * 4);
        const DSDTM::CovisibilityHost c = DSDTM::update_connection_host(m.t, d.kf);
        dsdtm_mapping_cov_result r{};
        r.n_cov = (int32_t)c.cov_kf.size(); r.n_connected = c.n_connected; r.overflow = r.n_cov > d.capacity;
        const size_t w = (size_t)std::min(r.n_cov, d.capacity);
        if (w) { memcpy(a.block + d.cov_kf, c.cov_kf.data(), w * 4); memcpy(a.block + d.cov_weight, c.cov_weight.data(), w * 4); }
        memcpy(a.block + d.result, &r, sizeof r);
    }
    return hipSuccess;
}

hipError_t mapping_window_launch(const MpWinArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (((size_t)a.block) & 7)) return hipErrorInvalidValue;
    for (int t = 0; t < a.n; ++t) {
        MpWinDev d;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        const size_t T = (size_t)1 << d.T_bits, E = (size_t)d.E;
        if (d.K > a.max_K || d.E > a.max_E || (long long)T > a.max_T || d.ocap > a.max_ocap || T < 2 * E) return hipErrorInvalidValue;
        const int32_t* local = (const int32_t*)(a.block + d.local);
        const int32_t* ent_off = (const int32_t*)(a.block + d.ent_off);
        if (local[0] != d.kf || ent_off[0] != 0 || ent_off[d.n_local] != d.E) return hipErrorInvalidValue;
        memset(a.block + d.table, 0xff, T * 8); memset(a.block + d.cell_lp, 0xff, T * 4);       // (the temporaries' room is there)
        memset(a.block + d.count, 0, E * 4); memset(a.block + d.cursor, 0, E * 4); memset(a.block + d.off, 0, (E + 1) * 4);
        memset(a.block + d.kfkey, 0, (size_t)d.K * 4); memset(a.block + d.kfwin, 0, (size_t)d.K * 4); memset(a.block + d.pairs, 0, (size_t)d.ocap * 8);
        HostMap m(d.points, d.kfs, d.slots, d.obs, d.feat, d.K, d.P);
        const DSDTM::BaWindowHost w = DSDTM::ba_window_host(m.t, d.kf, d.n_local - 1, local + 1, d.origin, d.kcap, d.pcap, d.ocap);
        memcpy(a.block + d.result, &w.result, sizeof w.result);
        if (!w.result.usable) continue;
        auto put = [](void* dst, const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); };
        put(d.kf_index, w.kf_index.data(), w.kf_index.size() * 4); put(d.kf_constant, w.kf_constant.data(), w.kf_constant.size());
        put(d.T_c2w, w.T_c2w.data(), w.T_c2w.size() * 8); put(d.point_index, w.point_index.data(), w.point_index.size() * 4);
        put(d.pts, w.points.data(), w.points.size() * 8); put(d.obs_kf, w.obs_kf.data(), w.obs_kf.size() * 4);
        put(d.obs_point, w.obs_point.data(), w.obs_point.size() * 4); put(d.obs_bearing, w.obs_bearing.data(), w.obs_bearing.size() * 8);
        put(d.obs_level, w.obs_level.data(), w.obs_level.size() * 4); put(d.obs_slot, w.obs_slot.data(), w.obs_slot.size() * 8);
    }
    return hipSuccess;
}

hipError_t mapping_commit_check_launch(const MpCommitArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (a.verdict & 7) || a.claims != a.verdict + 8) return hipErrorInvalidValue;
    memset(a.block + a.verdict, 0x7f, (size_t)a.claim_words * 4);
    unsigned long long verdict = MP_NO_OVERLAP;
    for (int t = 0; t < a.n; ++t) {
        MpCommitDev d;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        if (std::max(d.n_kf, d.n_points) > a.max_items) return hipErrorInvalidValue;
        int32_t* claim[2] = {(int32_t*)(a.block + d.claim_k), (int32_t*)(a.block + d.claim_p)};
        const int32_t* index[2] = {d.kf_index, d.point_index};
        const int count[2] = {d.n_kf, d.n_points}, limit[2] = {d.K, d.P};
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < count[c]; ++i) {
                if (index[c][i] < 0 || index[c][i] >= limit[c]) continue;
                int32_t& cell = claim[c][index[c][i]];                  // (records come in window order: the first claimer is the smallest)
                if (cell == 0x7f7f7f7f) cell = d.window;
                else if (cell != d.window) verdict = std::min(verdict, ((unsigned long long)(unsigned)cell << 32) | (unsigned)d.window);
            }
    }
    memcpy(a.block + a.verdict, &verdict, 8);
    return hipSuccess;
}

hipError_t mapping_commit_apply_launch(const MpCommitArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    for (int t = 0; t < a.n; ++t) {
        MpCommitDev d;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        HostMap m(d.points, d.kfs, d.slots, d.obs, nullptr, d.K, d.P);
        DSDTM::BaWindowHost w;
        w.kf_index.assign(d.kf_index, d.kf_index + d.n_kf); w.point_index.assign(d.point_index, d.point_index + d.n_points);
        w.obs_point.assign(d.obs_point, d.obs_point + d.n_obs); w.obs_slot.assign(d.obs_slot, d.obs_slot + d.n_obs);
        const DSDTM::MappingMapWritable wr = {m.p.data(), m.bad.data(), m.T.data(), m.off.data(), m.slots.data(), m.observes.data()};
        const DSDTM::BaCommitHost c = DSDTM::ba_commit_host(wr, w, d.T_c2w, d.pts, d.outlier);
        for (int i = 0; i < d.P; ++i) { d.points[i].x = m.p[3 * (size_t)i]; d.points[i].y = m.p[3 * (size_t)i + 1]; d.points[i].z = m.p[3 * (size_t)i + 2]; d.points[i].bad = m.bad[(size_t)i]; }
        for (int k = 0; k < d.K; ++k) memcpy(d.kfs[k].T, &m.T[12 * (size_t)k], 96);
        for (size_t s = 0; s < m.slots.size(); ++s) { d.slots[s] = m.slots[s]; d.obs[s] = m.observes[s] ? m.slots[s] : -1; }
        memset(a.block + d.went_bad, 0, (size_t)d.n_points * 4); memset(a.block + d.n_out, 0, (size_t)d.n_points * 4);
        dsdtm_mapping_commit_result r{};
        r.n_outliers = c.n_outliers; r.n_bad = (int32_t)c.bad_points.size(); r.overflow_bad = r.n_bad > d.bad_cap;
        const size_t n = (size_t)std::min(r.n_bad, d.bad_cap);
        if (n) memcpy(a.block + d.bad_list, c.bad_points.data(), n * 4);
        memcpy(a.block + d.result, &r, sizeof r);
    }
    return hipSuccess;
}

}  // namespace dsdtm
