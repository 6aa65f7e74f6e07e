// The fakes of the launch functions of dsdtm_amd/csrc/klt.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified and
// knows nothing of them (its own pyrdown_launch fills a level with 0x11, so every level but level 0 is flat and K5 skips it). That runtime runs queued operations only when something waits for
// them, so a fake first drains the stream (the upload queued in front of it then runs) and then does the kernel's work with the host
// functions of dsdtm_amd/host/dsdtm_klt_host.hpp on the very pointers, offsets and strides of the records: under AddressSanitizer an
// offset, a stride or a count that leaves its buffer shows up here, and the driver predicts every byte with the same functions.
// (homography.hip's launch is the fake of tests/fake_hip_homography.) Test infrastructure only.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fake_hip.h"
#include "fake_klt.h"
#include "klt.h"
#include "../../dsdtm_amd/host/dsdtm_klt_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_klt_fail(long nth) { g_fail = nth; }
long fake_klt_launches() { return g_launches; }

namespace dsdtm {

static bool enter(hipStream_t stream, hipError_t* e) {
    if (g_fail > 0 && --g_fail == 0) { *e = hipErrorUnknown; return false; }
    if (hipStreamSynchronize(stream) != hipSuccess) { *e = hipErrorUnknown; return false; }
    ++g_launches;
    return true;
}

hipError_t klt_ingest_launch(const KltIngest* recs, int n, int max_width, int max_height, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!recs || n <= 0) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    int seen_w = 0, seen_h = 0;
    for (int t = 0; t < n; ++t) {
        KltIngest r;
        memcpy(&r, recs + t, sizeof r);
        if (!r.src || !r.dst || r.sstride < r.width || r.dstride < r.width || r.width > max_width || r.height > max_height) return hipErrorInvalidValue;
        seen_w = r.width > seen_w ? r.width : seen_w; seen_h = r.height > seen_h ? r.height : seen_h;
        for (int y = 0; y < r.height; ++y) memcpy(r.dst + (size_t)y * r.dstride, r.src + (size_t)y * r.sstride, (size_t)r.width);
    }
    return seen_w == max_width && seen_h == max_height ? hipSuccess : hipErrorInvalidValue;
}

hipError_t klt_launch(const KltDev* recs, int n, int max_points, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (n <= 0 || max_points <= 0) return hipSuccess;          // (as klt.hip's: nothing to track)
    if (!recs) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    int seen = 0;
    for (int t = 0; t < n; ++t) {
        KltDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.n_points < 0 || r.n_points > max_points || r.levels < 1 || r.levels > DSDTM_KLT_MAX_LEVELS || !r.prev || !r.cur) return hipErrorInvalidValue;
        seen = r.n_points > seen ? r.n_points : seen;
        if (r.n_points == 0) continue;
        if (!r.points || !r.out_points || !r.status || !r.iterations) return hipErrorInvalidValue;
        DSDTM::KltLevel a[DSDTM_KLT_MAX_LEVELS], b[DSDTM_KLT_MAX_LEVELS];
        for (int l = 0; l < r.levels; ++l) {
            a[l] = DSDTM::KltLevel{r.prev + r.off[l], r.w[l], r.h[l], r.stride[l]};
            b[l] = DSDTM::KltLevel{r.cur + r.off[l], r.w[l], r.h[l], r.stride[l]};
        }
        DSDTM::KltParams P;
        P.window = r.window; P.iterations = r.max_iter; P.epsilon = std::sqrt(r.eps2); P.min_eig = r.min_eig;
        DSDTM::klt_flow_host(a, b, r.levels, r.n_points, r.points, r.guesses, P, r.out_points, r.status, r.iterations, r.residual);
    }
    return seen == max_points ? hipSuccess : hipErrorInvalidValue;
}

hipError_t klt_compact_launch(const KltCompact* recs, int n, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!recs || n <= 0) return hipErrorInvalidValue;
    if (!enter(stream, &e)) return e;
    for (int t = 0; t < n; ++t) {
        KltCompact r;
        memcpy(&r, recs + t, sizeof r);
        if (!r.rec || !r.n_tracked || !r.a || !r.b || r.n_points < 0) return hipErrorInvalidValue;
        int m = 0;
        for (int k = 0; k < r.n_points; ++k)
            if (r.status[k]) {
                r.a[2 * m] = r.points[2 * k]; r.a[2 * m + 1] = r.points[2 * k + 1];
                r.b[2 * m] = r.prev_points[2 * k]; r.b[2 * m + 1] = r.prev_points[2 * k + 1];
                ++m;
            }
        *r.n_tracked = m;
        r.rec->m = m >= r.min_tracked ? m : 0;
    }
    return hipSuccess;
}

}  // namespace dsdtm
