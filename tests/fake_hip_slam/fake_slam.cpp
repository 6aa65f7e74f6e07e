// Fake of the launch function of dsdtm_amd/csrc/aftertrack.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified and
// knows nothing of it (the map's own launches are the fakes of tests/fake_hip_trackmap and tests/fake_hip_localmap, the mapping
// thread's those of tests/fake_hip_mapping). That runtime runs queued operations only when something waits for them, so the fake first
// drains the stream. It turns each map's device arrays into plain arrays, answers with track_commit_host of
// dsdtm_amd/host/dsdtm_slam_host.hpp desc after desc through the block's offsets, and writes over the whole room of every temporary —
// under AddressSanitizer an offset, a count or a stale pointer that leaves its allocation shows up here. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "aftertrack.h"
#include "fake_hip.h"
#include "fake_slam.h"
#include "../../dsdtm_amd/host/dsdtm_slam_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_slam_fail(long nth) { g_fail = nth; }
long fake_slam_launches() { return g_launches; }

namespace dsdtm {

hipError_t aftertrack_commit_launch(const AtCommitArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    ++g_launches;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    if (!a.block || a.n_maps <= 0 || a.n <= 0 || (((size_t)a.block) & 7) || (a.descs & 7)) return hipErrorInvalidValue;
    std::vector<int> seen((size_t)a.n, 0);
    for (int mi = 0; mi < a.n_maps; ++mi) {
        AtMapDev m;
        memcpy(&m, a.block + (size_t)mi * sizeof m, sizeof m);
        if (m.S > a.max_S || m.n_descs <= 0) return hipErrorInvalidValue;
        const size_t P = (size_t)m.P, S = (size_t)m.S;
        std::vector<int32_t> found(m.found, m.found + P), slots(m.slots, m.slots + S);
        std::vector<uint8_t> bad(P), observes(S);
        for (size_t i = 0; i < P; ++i) bad[i] = m.points[i].bad ? 1 : 0;
        for (size_t s = 0; s < S; ++s) observes[s] = m.obs[s] >= 0 ? 1 : 0;
        DSDTM::TrackCommitMap t;
        t.n_points = m.P; t.found = found.data(); t.bad = bad.data(); t.n_slots_total = m.S; t.point_of_slot = slots.data(); t.observes = observes.data();
        const int32_t* list = (const int32_t*)(a.block + m.desc_list);
        size_t matches = 0;
        for (int di = 0; di < m.n_descs; ++di) {
            if (list[di] < 0 || list[di] >= a.n || seen[(size_t)list[di]]++ || (di && list[di] <= list[di - 1])) return hipErrorInvalidValue;
            AtDescDev d;
            memcpy(&d, a.block + a.descs + (size_t)list[di] * sizeof d, sizeof d);
            if (d.n_matches < 0 || d.n_matches > AT_THREADS || d.bad_cap < 0 || d.bad_cap > d.n_matches) return hipErrorInvalidValue;
            matches += (size_t)d.n_matches;
            const DSDTM::TrackCommitHost r = DSDTM::track_commit_host(t, a.threshold, d.n_matches, (const int32_t*)(a.block + d.point), (const double*)(a.block + d.norm));
            dsdtm_slam_commit_result res{};
            res.n_erased = r.n_erased; res.n_bad = (int32_t)r.bad_points.size();
            memset(a.block + d.bad_list, 0xEE, (size_t)d.bad_cap * 4);
            const size_t w = (size_t)std::min(res.n_bad, d.bad_cap);
            if (w) memcpy(a.block + d.bad_list, r.bad_points.data(), w * 4);
            if (d.n_matches) memcpy(a.block + d.found_after, r.found_after.data(), (size_t)d.n_matches * 4);
            memcpy(a.block + d.result, &res, sizeof res);
        }
        (void)matches;
        memset(a.block + m.stamp, 0xEE, (P + 7) / 8 * 8);           // (the temporaries' room is there)
        memset(a.block + m.n_new_bad, 0xEE, 4);
        for (size_t i = 0; i < P; ++i) { m.found[i] = found[i]; m.points[i].bad = bad[i]; }
        for (size_t s = 0; s < S; ++s) { m.slots[s] = slots[s]; m.obs[s] = observes[s] ? slots[s] : -1; }
    }
    for (int t = 0; t < a.n; ++t) if (seen[(size_t)t] != 1) return hipErrorInvalidValue;      // every desc belongs to exactly one map
    return hipSuccess;
}

hipError_t aftertrack_gather_launch(const AtGatherArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    ++g_launches;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (((size_t)a.block) & 7) || (a.descs & 7)) return hipErrorInvalidValue;
    for (int t = 0; t < a.n; ++t) {
        KeyframeTrackerDev r;
        AtGatherDev g;
        memcpy(&r, a.block + (size_t)t * sizeof r, sizeof r);
        memcpy(&g, a.block + a.descs + (size_t)t * sizeof g, sizeof g);
        if (g.kf < 0 || g.kf >= g.K || ((r.cur_p | r.kf_p | r.lkf) & 7)) return hipErrorInvalidValue;
        const size_t P = (size_t)g.P, K = (size_t)g.K;
        std::vector<double> p(3 * P), T(12 * K);
        std::vector<uint8_t> bad(P);
        std::vector<int32_t> ns(K);
        std::vector<int64_t> off(K);
        size_t S = 0;
        for (size_t i = 0; i < P; ++i) { p[3 * i] = g.points[i].x; p[3 * i + 1] = g.points[i].y; p[3 * i + 2] = g.points[i].z; bad[i] = g.points[i].bad ? 1 : 0; }
        for (size_t k = 0; k < K; ++k) {
            memcpy(&T[12 * k], g.kfs[k].T, 96); ns[k] = g.kfs[k].n_slots; off[k] = g.kfs[k].slot_off;
            S = std::max(S, (size_t)(g.kfs[k].slot_off + g.kfs[k].n_slots));
        }
        std::vector<int32_t> slots(g.slots, g.slots + S);
        DSDTM::TrackMapArrays m;
        m.sel.n_points = g.P; m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = g.K; m.sel.T_kf_w = T.data(); m.sel.n_slots = ns.data();
        m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
        const DSDTM::KeyframeDescHost h = DSDTM::gather_keyframe_desc_host(m, r.T_cur, r.n_valid, r.n_cur, (const int32_t*)(a.block + g.cur_point), g.kf, r.n_lkf,
                                                                           (const int32_t*)(a.block + g.local_kf));
        const size_t room = (size_t)ns[(size_t)g.kf];
        memset(a.block + r.kf_p, 0xEE, room * 24); memset(a.block + r.kf_bad, 0xEE, room);         // (the whole room is there)
        auto put = [&](uint64_t at, const void* src, size_t bytes) { if (bytes) memcpy(a.block + at, src, bytes); };
        put(r.cur_p, h.cur_p_world.data(), h.cur_p_world.size() * 8); put(r.cur_bad, h.cur_bad.data(), h.cur_bad.size());
        put(r.kf_p, h.kf_p_world.data(), h.kf_p_world.size() * 8); put(r.kf_bad, h.kf_bad.data(), h.kf_bad.size());
        put(r.lkf, h.local_kf_centre.data(), h.local_kf_centre.size() * 8);
        memcpy(r.T_kf, h.T_kf_w, 96);
        r.n_kf = (int32_t)h.kf_bad.size();
        memcpy(a.block + (size_t)t * sizeof r, &r, sizeof r);
    }
    return hipSuccess;
}

}  // namespace dsdtm
