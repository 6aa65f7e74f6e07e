// framediff_host_timer.cpp — frame_diff_host (dsdtm_amd/host/dsdtm_framediff_host.hpp: this repository's own C++, not OpenCV) timed on one
// host thread, as a shared object for tools/time_framediff.py, which alternates it with the device in one process.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I include -o tools/libframediff_host_timer.so tools/framediff_host_timer.cpp
#include <chrono>
#include <vector>

#include "../dsdtm_amd/host/dsdtm_framediff_host.hpp"

// mean microseconds per call over `reps` calls of one pair (mask written, n_features features looked up)
extern "C" double framediff_host_time_us(const uint8_t* a, const uint8_t* b, int w, int h, const double* H, int flags, int threshold, int maxval, uint8_t* mask,
                                         int n_features, const float* feature_px, uint8_t* feature_on_mask, int reps, int* n_foreground) {
    const auto t0 = std::chrono::steady_clock::now();
    int fg = 0;
    for (int k = 0; k < reps; ++k) fg += DSDTM::frame_diff_host(a, w, b, w, w, h, H, flags, threshold, maxval, mask, w, n_features, feature_px, feature_on_mask).n_foreground;
    const auto t1 = std::chrono::steady_clock::now();
    *n_foreground = reps ? fg / reps : 0;
    return std::chrono::duration<double, std::micro>(t1 - t0).count() / (reps ? reps : 1);
}
