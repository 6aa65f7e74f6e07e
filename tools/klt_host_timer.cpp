// klt_host_timer.cpp — klt_step_host (dsdtm_amd/host/dsdtm_klt_host.hpp: the repository's own C++, not OpenCV) on one host thread:
// wall per RunTrack at 640x480 (pyramid of the new image + the grid's flow + compaction), for tools/time_klt.py to set beside the device.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/klt_host_timer.cpp -o klt_host_timer && ./klt_host_timer [reps]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dsdtm_amd/host/dsdtm_klt_host.hpp"

static std::vector<uint8_t> frame(int w, int h, int shift) {
    std::vector<uint8_t> g((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double u = x - shift;
            g[(size_t)y * w + x] = (uint8_t)(128.0 + 45.0 * std::sin(u * 0.21 + y * 0.05) + 40.0 * std::cos(y * 0.17 - u * 0.07) + 30.0 * std::sin(u * 0.09) * std::cos(y * 0.11));
        }
    return g;
}

int main(int argc, char** argv) {
    const int w = 640, h = 480, reps = argc > 1 ? std::atoi(argv[1]) : 20;
    const std::vector<uint8_t> a = frame(w, h, 0), b = frame(w, h, 3);
    std::vector<std::vector<uint8_t>> s0, s1;
    std::vector<DSDTM::KltLevel> p0 = DSDTM::klt_pyramid_host(a.data(), w, h, w, 4, s0);
    double pyr = 0, flow = 0;
    int tracked = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<DSDTM::KltLevel> p1 = DSDTM::klt_pyramid_host(b.data(), w, h, w, 4, s1);
        const auto t1 = std::chrono::steady_clock::now();
        const DSDTM::KltStepHost hs = DSDTM::klt_step_host(p0.data(), p1.data(), 4);
        const auto t2 = std::chrono::steady_clock::now();
        pyr += std::chrono::duration<double, std::micro>(t1 - t0).count();
        flow += std::chrono::duration<double, std::micro>(t2 - t1).count();
        tracked = hs.n_tracked;
    }
    std::printf("klt_step_host 640x480 one thread: pyramid %.1f us + flow of 361 points %.1f us = %.1f us per RunTrack (%d tracked; no homography)\n",
                pyr / reps, flow / reps, (pyr + flow) / reps, tracked);
    return 0;
}
