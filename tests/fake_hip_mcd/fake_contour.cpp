// Fakes of the launch functions of dsdtm_amd/csrc/contour.hip for the fake HIP runtime of tests/fake_hip (used unmodified; the motion
// launches are the fakes of tests/fake_hip_motion). A fake first drains the stream, then walks every record: it reads every byte of the
// mask through the record's pitch, writes every element of the record's scratch arrays and the result, and the fill writes every byte of
// dst — under AddressSanitizer an offset, a pitch or a count that leaves its buffer shows up here. The result is mcd_box_host's
// (dsdtm_amd/host/dsdtm_mcd_host.hpp), so the driver can predict it. Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "../../dsdtm_amd/host/dsdtm_mcd_host.hpp"
#include "contour.h"
#include "fake_contour.h"
#include "fake_hip.h"

static std::atomic<long> g_fail{0}, g_contours{0}, g_fills{0};
void fake_contour_fail(long nth) { g_fail = nth; }
long fake_contour_launches() { return g_contours; }
long fake_contour_fill_launches() { return g_fills; }

namespace dsdtm {

hipError_t contour_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0 || max_pixels <= 0 || max_pixels > CONTOUR_MAX_PIXELS) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_contours;
    for (int t = 0; t < n; ++t) {
        ContourDev r;
        memcpy(&r, recs + t, sizeof r);
        if (r.width * r.height > max_pixels || r.src_pitch < r.width || !r.src || !r.result || !r.label || !r.ext || !r.roots || !r.keys) return hipErrorInvalidValue;
        const size_t px = (size_t)r.width * (size_t)r.height, cap = contour_list_cap(r.width, r.height);
        for (size_t k = 0; k < px; ++k) { r.label[k] = -1; r.ext[k] = r.ext[px + k] = r.ext[2 * px + k] = 0; }
        for (size_t k = 0; k < cap; ++k) { r.roots[k] = 0; r.keys[k] = 0; }
        const DSDTM::BoxResult b = DSDTM::mcd_box_host(r.src, r.width, r.height, r.src_pitch);
        ContourResult out;
        memcpy(out.box, b.box, sizeof out.box);
        out.area2 = b.area2; out.n_components = b.n_components; out.status = 0;
        *r.result = out;
    }
    return hipSuccess;
}

hipError_t contour_fill_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!recs || n <= 0 || max_pixels <= 0) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_fills;
    for (int t = 0; t < n; ++t) {
        ContourDev r;
        memcpy(&r, recs + t, sizeof r);
        if (!r.dst) continue;
        if (r.dst_pitch < r.width || r.width * r.height > max_pixels) return hipErrorInvalidValue;
        const int32_t* b = r.result->box;
        for (int y = 0; y < r.height; ++y)
            for (int x = 0; x < r.width; ++x) {
                const bool in = x >= b[0] && x < b[0] + b[2] && y >= b[1] && y < b[1] + b[3];
                r.dst[(size_t)y * (size_t)r.dst_pitch + (size_t)x] = in ? 255 : r.src[(size_t)y * (size_t)r.src_pitch + (size_t)x];
            }
    }
    return hipSuccess;
}

}  // namespace dsdtm
