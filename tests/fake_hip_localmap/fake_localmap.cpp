// Fakes of the launch functions of dsdtm_amd/csrc/localmap.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified
// and knows nothing of them. That runtime runs queued operations only when something waits for them, so each fake first drains the
// stream (the uploads queued in front of it then run). The apply fake copies its runs; the select fake turns every desc's device
// arrays into plain arrays and answers with select_local_map_host (dsdtm_amd/host/dsdtm_localmap_host.hpp) through the block's
// offsets — under AddressSanitizer an offset, a count or a stale pointer that leaves its allocation shows up here, and the driver
// can compare the answers with its own evaluation. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_localmap.h"
#include "localmap.h"
#include "../../dsdtm_amd/host/dsdtm_localmap_host.hpp"

static std::atomic<long> g_fail{0}, g_select{0}, g_apply{0};
void fake_localmap_fail(long nth) { g_fail = nth; }
long fake_localmap_select_launches() { return g_select; }
long fake_localmap_apply_launches() { return g_apply; }

namespace dsdtm {

hipError_t localmap_apply_launch(const LmApplyArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_apply;
    for (int i = 0; i < 2; ++i)
        if (a.words[i]) memcpy(a.dst[i], a.src[i], (size_t)a.words[i] * 4);
    return hipSuccess;
}

hipError_t localmap_select_launch(const LmSelectArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!a.block || a.n <= 0 || (((size_t)a.block) & 7)) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_select;
    const dsdtm_camera cam{a.fx, a.fy, a.cx, a.cy, a.fx, a.width, a.height};
    const dsdtm_localmap_params prm{a.n_local, a.boundary};
    for (int t = 0; t < a.n; ++t) {
        LmDescDev d;
        memcpy(&d, a.block + (size_t)t * sizeof d, sizeof d);
        if (d.K > a.max_K || d.P > a.max_P) return hipErrorInvalidValue;
        std::vector<double> p(3 * (size_t)d.P), T(12 * (size_t)d.K);
        std::vector<uint8_t> bad((size_t)d.P);
        std::vector<int32_t> ns((size_t)d.K);
        std::vector<int64_t> off((size_t)d.K);
        for (int i = 0; i < d.P; ++i) { p[3 * (size_t)i] = d.points[i].x; p[3 * (size_t)i + 1] = d.points[i].y; p[3 * (size_t)i + 2] = d.points[i].z; bad[(size_t)i] = d.points[i].bad ? 1 : 0; }
        for (int k = 0; k < d.K; ++k) { memcpy(&T[12 * (size_t)k], d.kfs[k].T, 96); ns[(size_t)k] = d.kfs[k].n_slots; off[(size_t)k] = d.kfs[k].slot_off; }
        DSDTM::LocalMapArrays m;
        m.n_points = d.P; m.p_world = p.data(); m.bad = bad.data(); m.n_keyframes = d.K; m.T_kf_w = T.data(); m.n_slots = ns.data();
        m.slot_offset = off.data(); m.point_of_slot = d.slots;
        for (int k = 0; k < d.K; ++k) ((unsigned long long*)(a.block + d.keys))[k] = ~0ull;      // (the keys' room is there)
        dsdtm_localmap_result r;
        DSDTM::select_local_map_host(cam, prm, m, d.T, (int32_t*)(a.block + d.kf), (double*)(a.block + d.kf_dist), d.capacity,
                                     (int32_t*)(a.block + d.point), (int32_t*)(a.block + d.point_kf), &r);
        memcpy(a.block + d.result, &r, sizeof r);
    }
    return hipSuccess;
}

}  // namespace dsdtm
