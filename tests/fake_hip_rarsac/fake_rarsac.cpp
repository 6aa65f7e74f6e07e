// The fake of the launch function of dsdtm_amd/csrc/rarsac.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified and
// knows nothing of it. That runtime runs queued operations only when something waits for them, so the fake first drains the stream
// (the upload queued in front of it then runs), then walks every record: it checks what the host derived (the sorted order, the
// table's ranges and prefix sums), reads every coordinate and writes the whole result and every status byte — under AddressSanitizer
// an offset or a count that leaves its buffer shows up here. What it writes is simple enough for the driver to predict: found = 0
// with fewer than 8 non-empty bins (reject only); else status[sorted i] = 1 where cur x >= prev x, n_inliers = m, best_hypothesis =
// seed & 0xFFFF, iterations_run = max_iterations, score = terminate (check: F[0]), F[j] = the sum of all coordinates + j (check: the
// caller's F), grid_probability_out[j] = binp[j] + the number of correspondences in bin j. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_rarsac.h"
#include "rarsac.h"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_rarsac_fail(long nth) { g_fail = nth; }
long fake_rarsac_launches() { return g_launches; }

namespace dsdtm {

hipError_t rarsac_launch(const RarsacDev* recs, int n, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    for (int t = 0; t < n; ++t) {
        RarsacDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.m < DSDTM_RARSAC_MIN_POINTS || r.m > DSDTM_RARSAC_MAX_POINTS || r.max_iterations < 1 || r.max_iterations > DSDTM_RARSAC_MAX_ITERATIONS || !r.out ||
            !r.status || !r.table || ((size_t)r.pt & 15) || !(r.terminate > 0) || !(r.inv_sigma2 > 0) || r.gr < 1 || r.gc < 1 || r.seed == 0)
            return hipErrorInvalidValue;
        RarsacTable tab;
        memcpy(&tab, r.table, sizeof tab);
        int nb = 0, total = 0;
        if (tab.start[0] != 0 || tab.start[RARSAC_GRID] != r.m) return hipErrorInvalidValue;
        for (int j = 0; j < RARSAC_GRID; ++j) {
            if (tab.start[j + 1] < tab.start[j]) return hipErrorInvalidValue;
            if (tab.start[j + 1] > tab.start[j]) {
                int w = (int)(tab.prior[j] * 1024.0);
                total += w < 1 ? 1 : w;
                if (tab.nbin[nb] != j || tab.cum[nb] != total) return hipErrorInvalidValue;
                ++nb;
            }
            // every correspondence of the range lies in bin j (R1, with the swapped divisors)
            for (int i = tab.start[j]; i < tab.start[j + 1]; ++i)
                if ((int)(r.pt[4 * i + 1] / (float)r.gc) * 10 + (int)(r.pt[4 * i] / (float)r.gr) != j) return hipErrorInvalidValue;
        }
        if (nb != r.nb || total != r.total) return hipErrorInvalidValue;
        dsdtm_rarsac_result o;
        memset(&o, 0x5A, sizeof o);
        if (!r.check && nb < 8) { o.found = 0; memcpy(r.out, &o, sizeof o); continue; }
        double sum = 0;
        for (int i = 0; i < 4 * r.m; ++i) sum += (double)r.pt[i];
        for (int i = 0; i < r.m; ++i) r.status[i] = r.pt[4 * i] >= r.pt[4 * i + 2] ? 1 : 0;
        for (int j = 0; j < 9; ++j) o.F[j] = r.check ? r.F[j] : (float)(sum + j);
        for (int j = 0; j < RARSAC_GRID; ++j) o.grid_probability_out[j] = tab.binp[j] + (double)(tab.start[j + 1] - tab.start[j]);
        o.found = 1; o.n_inliers = r.m; o.best_hypothesis = (int32_t)(r.seed & 0xFFFFu); o.iterations_run = r.check ? 0 : r.max_iterations;
        o.score = r.check ? (double)r.F[0] : r.terminate;
        memcpy(r.out, &o, sizeof o);
    }
    return hipSuccess;
}

}  // namespace dsdtm
