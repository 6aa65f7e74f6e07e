// undistort_host_timer.cpp — the single-thread baseline of tools/time_undistort.py: undistort_frame_host and undistort_points_host of
// dsdtm_amd/host/dsdtm_undistort_host.hpp (this repository's own straightforward C++, not OpenCV's SIMD remap) at 640 x 480 with the
// coefficients of Config/kinect.yaml. Prints microseconds per call (the median of `reps` calls).
//   g++ -O2 -std=c++14 -ffp-contract=off tools/undistort_host_timer.cpp -o undistort_host_timer && ./undistort_host_timer [reps]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dsdtm_amd/host/dsdtm_undistort_host.hpp"

template <class F>
static double median_us(int reps, F f) {
    std::vector<double> t;
    for (int r = 0; r < reps + 3; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 3) t.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 50, W = 640, H = 480;
    dsdtm_camera cam{};
    cam.fx = 517.306408f; cam.fy = 516.469215f; cam.cx = 318.643040f; cam.cy = 255.313989f; cam.width = W; cam.height = H;
    const float dist[5] = {0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f};
    std::vector<int32_t> map((size_t)W * H * 2);
    std::vector<uint8_t> g((size_t)W * H), go((size_t)W * H);
    std::vector<uint16_t> z((size_t)W * H), zo((size_t)W * H);
    for (size_t i = 0; i < g.size(); ++i) { g[i] = (uint8_t)(i * 2654435761u >> 24); z[i] = (uint16_t)(i * 40503u >> 4); }
    std::printf("undistort_map_host 640x480 %.1f us\n", median_us(std::max(3, reps / 10), [&] { DSDTM::undistort_map_host(cam, dist, map.data()); }));
    std::printf("undistort_frame_host gray+depth 640x480 %.1f us\n",
                median_us(reps, [&] { DSDTM::undistort_frame_host(map.data(), W, H, g.data(), W, go.data(), W, z.data(), W, zo.data(), W); }));
    std::printf("undistort_frame_host gray 640x480 %.1f us\n", median_us(reps, [&] { DSDTM::undistort_frame_host(map.data(), W, H, g.data(), W, go.data(), W); }));
    for (int trackers : {1, 64, 1024}) {
        const int n = 400 * trackers;
        std::vector<float> px(2 * (size_t)n), out(2 * (size_t)n);
        std::vector<double> b(3 * (size_t)n);
        for (int i = 0; i < n; ++i) { px[2 * i] = (float)((i * 37) % W) + 0.25f; px[2 * i + 1] = (float)((i * 91) % H) + 0.5f; }
        std::printf("undistort_points_host %d x 400 %.1f us\n", trackers, median_us(reps, [&] { DSDTM::undistort_points_host(cam, dist, n, px.data(), nullptr, out.data(), b.data()); }));
    }
    return go[1000] + zo[1000] == 70000 ? 1 : 0;
}
