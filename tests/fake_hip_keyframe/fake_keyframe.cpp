// Fake of the launch function of dsdtm_amd/csrc/keyframe.hip for the fake HIP runtime of tests/fake_hip, which is used
// unmodified and knows nothing of it. That runtime runs queued operations only when something waits for them, so the fake
// first drains the stream (the upload queued in front of it then runs), and then walks every tracker's record and arrays
// through the blob's offsets — under AddressSanitizer an offset or a count that leaves the upload shows up here — and leaves
// sums of what it read in the verdict, which the driver compares with its own. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_keyframe.h"
#include "keyframe.h"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_keyframe_fail(long nth) { g_fail = nth; }
long fake_keyframe_launches() { return g_launches; }

namespace dsdtm {

hipError_t need_keyframes_launch(const KeyframeArgs& a, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!a.blob || !a.verdict || a.n <= 0 || (((size_t)a.blob) & 7)) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;     // (the call waits right behind its read-back anyway)
    ++g_launches;
    for (int t = 0; t < a.n; ++t) {
        KeyframeTrackerDev r;
        memcpy(&r, a.blob + (size_t)t * sizeof r, sizeof r);
        auto sum_f64 = [&](uint64_t off, size_t n) { double s = 0; for (size_t i = 0; i < n; ++i) { double v; memcpy(&v, a.blob + off + 8 * i, 8); s += v; } return s; };
        auto sum_u8 = [&](uint64_t off, size_t n) { double s = 0; for (size_t i = 0; i < n; ++i) s += a.blob[off + i]; return s; };
        dsdtm_keyframe_verdict v;
        memset(&v, 0, sizeof v);
        v.need = r.n_valid; v.reason = a.prm.px_samples; v.n_px = r.n_kf; v.n_depth = r.n_cur; v.svo_kf = r.n_lkf;
        v.median_px = sum_f64(r.kf_p, 3 * (size_t)r.n_kf);
        v.median_depth = sum_f64(r.cur_p, 3 * (size_t)r.n_cur);
        v.min_depth = sum_u8(r.cur_bad, (size_t)r.n_cur) + 1000.0 * sum_u8(r.kf_bad, (size_t)r.n_kf);
        v.trans = sum_f64(r.lkf, 3 * (size_t)r.n_lkf);
        v.rot = r.T_cur[3] + r.T_kf[11] + (double)a.fx;
        a.verdict[t] = v;
    }
    return hipSuccess;
}

}  // namespace dsdtm
