// Fakes of the launch functions of dsdtm_amd/csrc/trackmap.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified
// and knows nothing of them (the selection's launches are the fakes of tests/fake_hip_localmap/fake_localmap.cpp). That runtime runs
// queued operations only when something waits for them, so each fake first drains the stream. The update fakes copy what the kernels
// copy; the flatten fake turns every desc's device arrays into plain arrays and answers with flatten_local_map_host
// (dsdtm_amd/host/dsdtm_trackmap_host.hpp) through the block's offsets — under AddressSanitizer an offset, a count or a stale pointer
// that leaves its allocation shows up here. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_trackmap.h"
#include "trackmap.h"
#include "../../dsdtm_amd/host/dsdtm_trackmap_host.hpp"

static std::atomic<long> g_fail{0}, g_flatten{0}, g_update{0};
void fake_trackmap_fail(long nth) { g_fail = nth; }
long fake_trackmap_flatten_launches() { return g_flatten; }
long fake_trackmap_update_launches() { return g_update; }

static bool enter(hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return false;
    return hipStreamSynchronize(stream) == hipSuccess;
}

namespace dsdtm {

hipError_t trackmap_apply_launch(const TmApplyArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    ++g_update;
    for (int i = 0; i < 4; ++i)
        if (a.words[i]) memcpy(a.dst[i], a.src[i], (size_t)a.words[i] * 4);
    return hipSuccess;
}

hipError_t trackmap_points_launch(const TmPointsArgs& a, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    ++g_update;
    for (int i = 0; i < a.n; ++i) {
        const int idx = a.first + i;
        LmPointDev& pt = a.points[idx];
        pt.x = a.xyz[3 * (size_t)i]; pt.y = a.xyz[3 * (size_t)i + 1]; pt.z = a.xyz[3 * (size_t)i + 2];
        if (a.bad) pt.bad = a.bad[i] ? 1 : 0; else if (idx >= a.old_count) pt.bad = 0;
        if (a.found) a.found_dst[idx] = a.found[i]; else if (idx >= a.old_count) a.found_dst[idx] = 0;
    }
    return hipSuccess;
}

hipError_t trackmap_found_launch(int32_t* found_dst, const int32_t* index, const int32_t* found, int n, hipStream_t stream) {
    if (!enter(stream)) return hipErrorUnknown;
    ++g_update;
    for (int i = 0; i < n; ++i) found_dst[index[i]] = found[i];
    return hipSuccess;
}

hipError_t trackmap_flatten_launch(const TmLocalArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (((size_t)a.block) & 7) || (a.descs & 7)) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_flatten;
    for (int t = 0; t < a.n; ++t) {
        LmDescDev d;
        TmDescDev q;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        memcpy(&q, a.block + a.descs + (size_t)t * sizeof q, sizeof q);
        if (d.K > a.max_K || d.capacity > a.max_cap || q.ocap > a.max_ocap) return hipErrorInvalidValue;
        dsdtm_localmap_result sel;
        memcpy(&sel, a.block + d.result, sizeof sel);
        const int32_t m = sel.n_points < d.capacity ? sel.n_points : d.capacity;
        std::vector<double> p(3 * (size_t)d.P), T(12 * (size_t)d.K);
        std::vector<uint8_t> bad((size_t)d.P);
        std::vector<int32_t> ns((size_t)d.K);
        std::vector<int64_t> off((size_t)d.K);
        size_t S = 0;
        for (int i = 0; i < d.P; ++i) { p[3 * (size_t)i] = d.points[i].x; p[3 * (size_t)i + 1] = d.points[i].y; p[3 * (size_t)i + 2] = d.points[i].z; bad[(size_t)i] = d.points[i].bad ? 1 : 0; }
        for (int k = 0; k < d.K; ++k) {
            memcpy(&T[12 * (size_t)k], d.kfs[k].T, 96); ns[(size_t)k] = d.kfs[k].n_slots; off[(size_t)k] = d.kfs[k].slot_off;
            S = std::max(S, (size_t)(d.kfs[k].slot_off + d.kfs[k].n_slots));
        }
        std::vector<uint8_t> observes(S);
        std::vector<float> px(2 * S);
        std::vector<int32_t> level(S);
        std::vector<double> bearing(3 * S);
        for (size_t s = 0; s < S; ++s) {
            observes[s] = q.obs[s] >= 0 ? 1 : 0;
            if (q.obs[s] >= 0 && q.obs[s] != d.slots[s]) return hipErrorInvalidValue;      // (an observing slot names its own point)
            px[2 * s] = q.feat[s].px[0]; px[2 * s + 1] = q.feat[s].px[1]; level[s] = q.feat[s].level;
            memcpy(&bearing[3 * s], q.feat[s].bearing, 24);
        }
        DSDTM::TrackMapArrays w;
        w.sel.n_points = d.P; w.sel.p_world = p.data(); w.sel.bad = bad.data(); w.sel.n_keyframes = d.K; w.sel.T_kf_w = T.data(); w.sel.n_slots = ns.data();
        w.sel.slot_offset = off.data(); w.sel.point_of_slot = d.slots;
        w.found = q.found; w.observes = observes.data(); w.px_xy = px.data(); w.level = level.data(); w.bearing = bearing.data();
        for (int i = 0; i < d.capacity; ++i) { ((int32_t*)(a.block + q.count))[i] = 0; ((int32_t*)(a.block + q.cursor))[i] = 0; }      // (the temporaries' room is there)
        for (int j = 0; j < q.ocap; ++j) ((uint64_t*)(a.block + q.pairs))[j] = 0;
        TmExtResult ext{};
        DSDTM::flatten_local_map_host(w, m, (const int32_t*)(a.block + d.point), q.ocap, (double*)(a.block + q.mp_world), (int32_t*)(a.block + q.mp_found),
                                      a.block + q.mp_bad, (int32_t*)(a.block + q.obs_offset), (int32_t*)(a.block + q.obs_kf), (float*)(a.block + q.obs_px),
                                      (int32_t*)(a.block + q.obs_level), (double*)(a.block + q.obs_bearing), &ext.n_obs);
        ext.overflow_obs = ext.n_obs > q.ocap ? 1 : 0; ext.straddle = -1;
        memcpy(a.block + q.ext, &ext, sizeof ext);
    }
    return hipSuccess;
}

}  // namespace dsdtm
