// The fakes of the three launch functions of dsdtm_amd/csrc/undistort.hip for the fake HIP runtime of tests/fake_hip, which is used
// unmodified and knows nothing of them. That runtime runs queued operations only when something waits for them, so a fake first drains
// the stream (the upload queued in front of it then runs) and then does the kernel's work with the host functions of
// dsdtm_amd/host/dsdtm_undistort_host.hpp on the very pointers and strides of the records: under AddressSanitizer an offset, a stride or
// a count that leaves its buffer shows up here, and the driver predicts every byte with the same functions. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_undistort.h"
#include "undistort.h"
#include "../../dsdtm_amd/host/dsdtm_undistort_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_undistort_fail(long nth) { g_fail = nth; }
long fake_undistort_launches() { return g_launches; }

namespace dsdtm {

static dsdtm_camera camera_of(const UndistortModel& m, int w, int h) {
    dsdtm_camera cam{};
    cam.fx = (float)m.fx; cam.fy = (float)m.fy; cam.cx = (float)m.cx; cam.cy = (float)m.cy; cam.width = w; cam.height = h;      // (exact: they were floats)
    return cam;
}

hipError_t undistort_map_launch(const UndistortModel& m, int w, int h, int32_t* map, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!map || w < DSDTM_UNDISTORT_MIN_SIDE || h < DSDTM_UNDISTORT_MIN_SIDE || w > DSDTM_UNDISTORT_MAX_SIDE || h > DSDTM_UNDISTORT_MAX_SIDE) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    const float dist[5] = {(float)m.k1, (float)m.k2, (float)m.p1, (float)m.p2, (float)m.k3};
    const dsdtm_camera cam = camera_of(m, w, h);
    DSDTM::undistort_map_host(cam, dist, map);
    return hipSuccess;
}

hipError_t undistort_frames_launch(const UndistortFrameDev* frames, int n, int max_w, int max_h, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!frames || n <= 0 || n > DSDTM_UNDISTORT_MAX_FRAMES) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    int seen_w = 0, seen_h = 0;
    for (int t = 0; t < n; ++t) {
        UndistortFrameDev f;
        memcpy(&f, frames + t, sizeof f);
        if (!f.map || !f.gray_src || !f.gray_dst || !f.depth_src != !f.depth_dst || f.gray_src_stride < f.w || f.gray_dst_stride < f.w ||
            (f.depth_src && (f.depth_src_stride < f.w || f.depth_dst_stride < f.w)) || f.w > max_w || f.h > max_h)
            return hipErrorInvalidValue;
        seen_w = f.w > seen_w ? f.w : seen_w; seen_h = f.h > seen_h ? f.h : seen_h;
        DSDTM::undistort_frame_host(f.map, f.w, f.h, f.gray_src, f.gray_src_stride, f.gray_dst, f.gray_dst_stride, f.depth_src, f.depth_src_stride,
                                    f.depth_dst, f.depth_dst_stride);
    }
    return seen_w == max_w && seen_h == max_h ? hipSuccess : hipErrorInvalidValue;      // the grid is sized by the largest frame, no larger
}

hipError_t undistort_points_launch(const UndistortModel& m, float fx, float fy, float cx, float cy, int n, const float* px_in, const uint8_t* skip,
                                   float* px_out, double* bearing, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (n <= 0 || n > DSDTM_UNDISTORT_MAX_POINTS || !px_in || !skip || !px_out || !bearing || (double)fx != m.fx || (double)fy != m.fy ||
        (double)cx != m.cx || (double)cy != m.cy)
        return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    const float dist[5] = {(float)m.k1, (float)m.k2, (float)m.p1, (float)m.p2, (float)m.k3};
    const dsdtm_camera cam = camera_of(m, 0, 0);
    DSDTM::undistort_points_host(cam, dist, n, px_in, skip, px_out, bearing);
    return hipSuccess;
}

}  // namespace dsdtm
