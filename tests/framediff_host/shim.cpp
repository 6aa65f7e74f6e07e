// frame_diff_host and warp_perspective_host (dsdtm_amd/host/dsdtm_framediff_host.hpp) behind C entries, for tests/framediff_cases.py.
// Test infrastructure only; it links nothing.
#include <cstring>

#include "../../dsdtm_amd/host/dsdtm_framediff_host.hpp"

// stages: 5 packed w x h images (warped, t, e, o, f); counts: n_foreground, n_flagged. Returns 0 where F1 refuses (nothing written).
extern "C" int frame_diff_host_c(const uint8_t* a, int a_stride, const uint8_t* b, int b_stride, int w, int h, const double* H, int flags, int threshold,
                                 int maxval, uint8_t* mask, int mask_stride, int n_features, const float* feature_px, uint8_t* feature_on_mask,
                                 uint8_t* stages, double* M, int32_t* counts) {
    const DSDTM::FrameDiffHost r = DSDTM::frame_diff_host(a, a_stride, b, b_stride, w, h, H, flags, threshold, maxval, mask, mask_stride, n_features,
                                                          feature_px, feature_on_mask);
    if (!r.ok) return 0;
    const size_t px = (size_t)w * (size_t)h;
    const std::vector<uint8_t>* s[5] = {&r.warped, &r.t, &r.e, &r.o, &r.f};
    for (int k = 0; k < 5; ++k) std::memcpy(stages + (size_t)k * px, s[k]->data(), px);
    std::memcpy(M, r.M, sizeof r.M);
    counts[0] = r.n_foreground; counts[1] = r.n_flagged;
    return 1;
}

extern "C" int warp_perspective_host_c(const uint8_t* b, int b_stride, int w, int h, const double* H, int flags, uint8_t* warped, int warped_stride, double* M) {
    double m[9];
    if (!DSDTM::framediff_matrix_host(H, flags, m)) return 0;
    DSDTM::warp_perspective_host(b, w, h, b_stride, m, warped, warped_stride);
    std::memcpy(M, m, sizeof m);
    return 1;
}
