// Fakes of the launch functions of dsdtm_amd/csrc/motion.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified
// and knows nothing of them. That runtime runs queued operations only when something waits for them, so a fake first drains the
// stream (the upload queued in front of it then runs), then walks every record: it reads every byte of the image through the
// record's stride, every float of the source generation and the feature coordinates, and writes every float of the destination
// generation, every byte of the mask and the flags — under AddressSanitizer an offset, a pitch or a count that leaves its buffer
// shows up here. What it writes is simple enough for the driver to predict: dst = src + 1 (1 from a NULL source); mask = 255 where the
// image byte is >= 128; flag = mask at the rounded feature == 255. Test infrastructure only.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_motion.h"
#include "motion.h"

static std::atomic<long> g_fail{0}, g_steps{0}, g_features{0};
void fake_motion_fail(long nth) { g_fail = nth; }
long fake_motion_step_launches() { return g_steps; }
long fake_motion_feature_launches() { return g_features; }

namespace dsdtm {

hipError_t motion_step_launch(const MotionStepDev* recs, int n, int tiles_x, int tiles_y, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0 || tiles_x <= 0 || tiles_y <= 0) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_steps;
    for (int t = 0; t < n; ++t) {
        MotionStepDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.mw != r.width / 4 || r.mh != r.height / 4 || (r.mw + 15) / 16 > tiles_x || (r.mh + 15) / 16 > tiles_y || !r.dst || r.src == r.dst) return hipErrorInvalidValue;
        const size_t cells = (size_t)r.mw * (size_t)r.mh;
        for (size_t k = 0; k < 12 * cells; ++k) r.dst[k] = (r.src ? r.src[k] : 0.0f) + 1.0f;
        if (r.image && r.img_stride < r.width) return hipErrorInvalidValue;
        if (r.mask && (r.mask_pitch < r.width || (r.mask_pitch & 3) || (((size_t)r.mask) & 3))) return hipErrorInvalidValue;
        for (int y = 0; y < r.height; ++y)
            for (int x = 0; x < r.width; ++x) {
                const uint8_t p = r.image ? r.image[(size_t)y * (size_t)r.img_stride + (size_t)x] : 0;
                if (r.mask) r.mask[(size_t)y * (size_t)r.mask_pitch + (size_t)x] = p >= 128 ? 255 : 0;
            }
    }
    return hipSuccess;
}

hipError_t motion_features_launch(const MotionStepDev* recs, int n, int max_features, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0 || max_features <= 0) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_features;
    for (int t = 0; t < n; ++t) {
        MotionStepDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.n_feat > max_features || (r.n_feat > 0 && (!r.feat || !r.flags || !r.mask))) return hipErrorInvalidValue;
        for (int f = 0; f < r.n_feat; ++f) {
            const int x = (int)nearbyintf(r.feat[2 * f]), y = (int)nearbyintf(r.feat[2 * f + 1]);
            if (x < 0 || x >= r.width || y < 0 || y >= r.height) return hipErrorInvalidValue;
            r.flags[f] = r.mask[(size_t)y * (size_t)r.mask_pitch + (size_t)x] == 255 ? 1 : 0;
        }
    }
    return hipSuccess;
}

}  // namespace dsdtm
