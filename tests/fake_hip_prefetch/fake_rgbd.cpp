// Fakes of the two launch functions of dsdtm_amd/csrc/rgbd.hip for the fake HIP runtime of tests/fake_hip, which is used
// unmodified and knows nothing of them. That runtime runs queued operations only when something waits for them, and the
// only queued operation with a payload it offers to outsiders is a copy — so the faked depth conversion is a queued copy
// per row: the frame's plane receives the RAW 16-bit values of the source as it is WHEN THE COPY RUNS (first half of every
// float row), which is what the tests are about: a staged source that was overwritten too early shows up in the plane.
// The faked lift hands back the raw value at the rounded pixel (0 -> -1). Test infrastructure only.
#include <atomic>
#include <cmath>
#include <cstdint>

#include "fake_hip.h"
#include "fake_rgbd.h"
#include "kernels.h"

static std::atomic<long> g_fail_depth{0}, g_fail_lift{0}, g_depth_launches{0};   // (two contexts launch from two threads)
static std::atomic<float> g_inv_scale{0.0f};
void fake_rgbd_fail(long depth_nth, long lift_nth) { g_fail_depth = depth_nth; g_fail_lift = lift_nth; }
long fake_rgbd_depth_launches() { return g_depth_launches; }
float fake_rgbd_last_inv_scale() { return g_inv_scale; }

namespace dsdtm {

hipError_t depth_ingest_launch(const uint16_t* src, int src_stride, float* dst, int w, int h, float inv_scale, int, hipStream_t stream) {
    if (g_fail_depth > 0 && --g_fail_depth == 0) return hipErrorUnknown;
    if (!src || !dst || src_stride < w || (((size_t)dst) & 15)) return hipErrorInvalidValue;
    for (int y = 0; y < h; ++y)
        if (hipMemcpyAsync(dst + (size_t)y * w, src + (size_t)y * src_stride, (size_t)w * 2, hipMemcpyHostToDevice, stream) != hipSuccess)
            return hipErrorUnknown;
    ++g_depth_launches;
    g_inv_scale = inv_scale;
    return hipSuccess;
}

hipError_t lift_launch(const LiftArgs& a, hipStream_t stream) {
    if (g_fail_lift > 0 && --g_fail_lift == 0) return hipErrorUnknown;
    // (dsdtm_frame_lift waits for the stream right behind the launch: draining it here runs the event waits queued in front)
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    for (int i = 0; i < a.n; ++i) {
        const int x = (int)std::lrintf(a.px_xy[2 * i]), y = (int)std::lrintf(a.px_xy[2 * i + 1]);
        float d = -1.0f;
        if (x >= 0 && x < a.w && y >= 0 && y < a.h) {
            const uint16_t raw = ((const uint16_t*)(a.depth + (size_t)y * a.w))[x];
            if (raw) d = (float)raw;
        }
        a.depth_out[i] = d;
        a.p_world[3 * i] = a.T[3]; a.p_world[3 * i + 1] = a.T[7]; a.p_world[3 * i + 2] = a.T[11];
    }
    return hipSuccess;
}

}  // namespace dsdtm
