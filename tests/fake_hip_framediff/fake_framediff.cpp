// The fakes of the three launch functions of dsdtm_amd/csrc/framediff.hip for the fake HIP runtime of tests/fake_hip, which is used
// unmodified and knows nothing of them. That runtime runs queued operations only when something waits for them, so a fake first drains
// the stream (the upload queued in front of it then runs) and then does the kernel's work with the host functions of
// dsdtm_amd/host/dsdtm_framediff_host.hpp on the very pointers and strides of the records: under AddressSanitizer an offset, a stride or
// a count that leaves its buffer shows up here, and the driver predicts every byte with the same functions. Test infrastructure only.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_framediff.h"
#include "framediff.h"
#include "../../dsdtm_amd/host/dsdtm_framediff_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_framediff_fail(long nth) { g_fail = nth; }
long fake_framediff_launches() { return g_launches; }

namespace dsdtm {

static bool enter(hipStream_t stream, hipError_t* e) {
    if (g_fail > 0 && --g_fail == 0) { *e = hipErrorUnknown; return false; }
    if (hipStreamSynchronize(stream) != hipSuccess) { *e = hipErrorUnknown; return false; }
    ++g_launches;
    return true;
}

hipError_t framediff_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!recs || n <= 0 || n > DSDTM_FRAMEDIFF_MAX_STEPS) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    int seen_w = 0, seen_h = 0;
    for (int t = 0; t < n; ++t) {
        FrameDiffDev r;
        memcpy(&r, recs + t, sizeof r);
        if (!r.a || !r.b || !r.n_foreground || r.a_stride < r.w || r.b_stride < r.w || (r.mask && r.mask_stride < r.w) || (r.warped && r.warped_stride < r.w) ||
            r.w > max_w || r.h > max_h || r.maxval < 1 || r.maxval > 255 || (r.n_feat > 0 && (!r.mask || !r.feat || !r.flags)))
            return hipErrorInvalidValue;
        if (*r.n_foreground != 0) return hipErrorInvalidValue;          // the counter starts at zero
        seen_w = r.w > seen_w ? r.w : seen_w; seen_h = r.h > seen_h ? r.h : seen_h;
        // (M is final: the inverse-map flag makes frame_diff_host take it as it is)
        const DSDTM::FrameDiffHost h = DSDTM::frame_diff_host(r.a, r.a_stride, r.b, r.b_stride, r.w, r.h, r.M, DSDTM_FRAMEDIFF_INVERSE_MAP, r.threshold, r.maxval,
                                                              r.mask, r.mask_stride);
        if (!h.ok) return hipErrorInvalidValue;
        if (r.warped) for (int y = 0; y < r.h; ++y) memcpy(r.warped + (size_t)y * r.warped_stride, h.warped.data() + (size_t)y * r.w, (size_t)r.w);
        *r.n_foreground = h.n_foreground;
    }
    return seen_w == max_w && seen_h == max_h ? hipSuccess : hipErrorInvalidValue;      // the grid is sized by the largest pair, no larger
}

hipError_t framediff_features_launch(const FrameDiffDev* recs, int n, int max_features, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!recs || n <= 0 || max_features <= 0) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    int seen = 0;
    for (int t = 0; t < n; ++t) {
        FrameDiffDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.n_feat < 0 || r.n_feat > max_features) return hipErrorInvalidValue;
        seen = r.n_feat > seen ? r.n_feat : seen;
        for (int f = 0; f < r.n_feat; ++f) {
            const size_t x = (size_t)std::nearbyintf(r.feat[2 * (size_t)f]), y = (size_t)std::nearbyintf(r.feat[2 * (size_t)f + 1]);
            r.flags[f] = r.mask[y * (size_t)r.mask_stride + x] == 255;
        }
    }
    return seen == max_features ? hipSuccess : hipErrorInvalidValue;
}

hipError_t framediff_warp_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!recs || n <= 0 || n > DSDTM_FRAMEDIFF_MAX_STEPS) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    int seen_w = 0, seen_h = 0;
    for (int t = 0; t < n; ++t) {
        FrameDiffDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.a || !r.b || !r.warped || r.mask || r.b_stride < r.w || r.warped_stride < r.w || r.w > max_w || r.h > max_h) return hipErrorInvalidValue;
        seen_w = r.w > seen_w ? r.w : seen_w; seen_h = r.h > seen_h ? r.h : seen_h;
        DSDTM::warp_perspective_host(r.b, r.w, r.h, r.b_stride, r.M, r.warped, r.warped_stride);
    }
    return seen_w == max_w && seen_h == max_h ? hipSuccess : hipErrorInvalidValue;
}

}  // namespace dsdtm
