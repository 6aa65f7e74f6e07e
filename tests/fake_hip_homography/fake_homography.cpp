// The fake of the launch function of dsdtm_amd/csrc/homography.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified
// and knows nothing of it. That runtime runs queued operations only when something waits for them, so the fake first drains the
// stream (the upload queued in front of it then runs), then walks every record: it reads every coordinate of both point arrays and
// writes the whole result and every byte of the mask — under AddressSanitizer an offset or a count that leaves its buffer shows up
// here. What it writes is simple enough for the driver to predict: found = (m > 4) and, with it, n_inliers = m, H[j] = the sum of all
// A coordinates + j, rounds = rounds_max, best_hypothesis = seed & 0xFFFF, cost_before = thr2, cost_after = left,
// mask[i] = 1 where A's x is at least B's x. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_homography.h"
#include "homography.h"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_homography_fail(long nth) { g_fail = nth; }
long fake_homography_launches() { return g_launches; }

namespace dsdtm {

hipError_t homography_launch(const HomographyDev* recs, int n, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    for (int t = 0; t < n; ++t) {
        HomographyDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.m < 0 || r.m > DSDTM_HOMOGRAPHY_MAX_POINTS || r.rounds_max < 1 || r.rounds_max > HOMOGRAPHY_MAX_ROUNDS || !r.out || !r.mask ||
            (((size_t)r.a | (size_t)r.b) & 7) || !(r.thr2 > 0) || !(r.left > 0))
            return hipErrorInvalidValue;
        dsdtm_homography_result o;
        memset(&o, 0x5A, sizeof o);
        o.found = r.m > 4 ? 1 : 0;
        double sum = 0;
        for (int i = 0; i < 2 * r.m; ++i) sum += (double)r.a[i];
        for (int i = 0; i < r.m; ++i) r.mask[i] = r.a[2 * i] >= r.b[2 * i] ? 1 : 0;
        for (int j = 0; j < 9; ++j) o.H[j] = sum + j;
        o.n_inliers = r.m; o.rounds = r.rounds_max; o.best_hypothesis = (int32_t)(r.seed & 0xFFFFu); o.refit_iterations = 0;
        o.cost_before = r.thr2; o.cost_after = r.left;
        memcpy(r.out, &o, sizeof o);
    }
    return hipSuccess;
}

}  // namespace dsdtm
