// Fake of the launch function of dsdtm_amd/csrc/newkf.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified and knows
// nothing of it. That runtime runs queued operations only when something waits for them, so the fake first drains the stream (the
// upload queued in front of it then runs) and then answers every tracker with create_keyframe_host (dsdtm_amd/host/dsdtm_newkf_host.hpp)
// on what it finds behind the record's DEVICE addresses — under AddressSanitizer an offset, a pitch or a count that leaves the upload or
// the caller's array shows up here — and writes the results with the guards of the real kernel. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_newkf.h"
#include "newkf.h"
#include "../../dsdtm_amd/host/dsdtm_newkf_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
static std::vector<dsdtm::NewkfTrackerDev> g_last;
void fake_newkf_fail(long nth) { g_fail = nth; }
long fake_newkf_launches() { return g_launches; }
const void* fake_newkf_seen(int t, int which) {
    const dsdtm::NewkfTrackerDev& r = g_last.at((size_t)t);
    return which == 0 ? (const void*)r.cell_score : which == 1 ? (const void*)r.depth : which == 2 ? (const void*)r.dyn : (const void*)r.cell_x;
}

namespace dsdtm {

hipError_t newkf_make_launch(const NewkfArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!a.trackers || a.n <= 0 || (((size_t)a.trackers) & 7)) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;     // (the call waits right behind its read-back anyway)
    ++g_launches;
    g_last.assign(a.trackers, a.trackers + a.n);
    dsdtm_camera cam{};
    cam.fx = a.fx; cam.fy = a.fy; cam.cx = a.cx; cam.cy = a.cy;
    for (int t = 0; t < a.n; ++t) {
        const NewkfTrackerDev& r = a.trackers[t];
        dsdtm_newkf_desc d{};
        d.cell_score = r.cell_score; d.cell_x = r.cell_x; d.cell_y = r.cell_y; d.cell_level = r.cell_level;
        d.n_existing = r.n_existing; d.first_point_index = r.first_point_index;
        d.px_xy = r.px_xy; d.level = r.level; d.bearing = r.bearing; d.has_point = r.has_point; d.initial = r.initial; d.point_index = r.point_index;
        d.depth = r.depth; d.depth_stride = r.depth_stride; d.depth_scale = 1.0f / r.inv_depth_scale;      // (the drivers use powers of two)
        d.dyn_mask = r.dyn; d.dyn_stride = r.dyn_stride; d.T_c2w = r.T;
        const DSDTM::NewKeyframeHost o = DSDTM::create_keyframe_host(cam, a.prm, d);
        for (int i = 0; i < o.n_slots && i < r.out_slots; ++i) {
            r.o_point_of_slot[i] = o.point_of_slot[(size_t)i]; r.o_observes[i] = o.observes[(size_t)i]; r.o_level[i] = o.level[(size_t)i];
            r.o_depth[i] = o.depth_of_slot[(size_t)i];
            memcpy(r.o_px_xy + 2 * i, &o.px_xy[2 * (size_t)i], 8); memcpy(r.o_bearing + 3 * i, &o.bearing[3 * (size_t)i], 24);
        }
        for (int i = 0; i < o.n_new_points && i < r.out_points; ++i) memcpy(r.o_p_world + 3 * i, &o.new_p_world[3 * (size_t)i], 24);
        r.counts[0] = o.n_new; r.counts[1] = o.n_slots; r.counts[2] = o.n_new_points;
        r.counts[3] = (o.n_slots > r.slot_cap || o.n_new_points > r.point_cap || (r.bad_cap >= 0 && o.n_new_points > r.bad_cap)) ? 1 : 0;
    }
    return hipSuccess;
}

}  // namespace dsdtm
