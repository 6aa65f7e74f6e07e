// example_rarsac.cpp — the pipeline of Test/test_Optimizer.cpp:91-106 without OpenCV: pyramidal LK (dsdtm_klt_flow of libdsdtm_amd_klt.so),
// then epipolar outlier rejection (DSDTM::Rarsac_base of dsdtm_rarsac_host.hpp), then the caller's ReduceFeatures.
//
//   g++ -O2 -std=c++14 -ffp-contract=off example_rarsac.cpp ../csrc/libdsdtm_amd_rarsac.so ../csrc/libdsdtm_amd_klt.so
//       -Wl,-rpath,../csrc -L/opt/rocm/lib -lamdhip64 -o example_rarsac
//
// A smooth scene moves by (2, 1) pixels between the previous and the current image; a tenth of the tracked points is then sent
// somewhere else. The program exits with 0 only when the device's RejectFundamental equals the host function's in every byte of the
// status and every bit of the grid, and ReduceFeatures leaves what the status marks.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/dsdtm_amd_klt.h"
#include "dsdtm_rarsac_host.hpp"

static std::vector<uint8_t> frame(int w, int h, double dx, double dy) {
    std::vector<uint8_t> g((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double u = x - dx, v = y - dy;
            const double s = 128.0 + 50.0 * std::sin(u * 0.11 + v * 0.07) + 40.0 * std::cos(v * 0.13 - u * 0.05) + 30.0 * std::sin(u * 0.31) * std::cos(v * 0.29);
            g[(size_t)y * w + x] = (uint8_t)(s < 0.0 ? 0.0 : (s > 255.0 ? 255.0 : s));
        }
    return g;
}

int main() {
    const int w = 640, h = 480;
    try {
        const std::vector<uint8_t> prev_img = frame(w, h, 0.0, 0.0), cur_img = frame(w, h, 2.0, 1.0);
        std::vector<float> pts;
        for (int y = 40; y < 440; y += 40)
            for (int x = 40; x < 600; x += 40) { pts.push_back((float)x); pts.push_back((float)y); }
        const int n = (int)pts.size() / 2;
        std::vector<float> out(pts.size());
        std::vector<uint8_t> tracked((size_t)n);
        dsdtm_klt_ctx* k = nullptr;
        if (dsdtm_klt_create(0, &k) != DSDTM_OK) { std::printf("no device: %s\n", dsdtm_klt_last_error(nullptr)); return 1; }
        dsdtm_klt_flow_desc fd{};
        fd.prev = prev_img.data(); fd.cur = cur_img.data(); fd.width = w; fd.height = h; fd.prev_stride = fd.cur_stride = w;
        fd.n_points = n; fd.points = pts.data(); fd.out_points = out.data(); fd.status = tracked.data();
        const int rc = dsdtm_klt_flow(k, 1, &fd);
        if (rc != DSDTM_OK) { std::printf("dsdtm_klt_flow: %s\n", dsdtm_klt_last_error(k)); dsdtm_klt_destroy(k); return 1; }
        dsdtm_klt_destroy(k);
        std::vector<DSDTM::RarsacPoint2f> cur, prev;
        for (int i = 0; i < n; ++i) {
            if (!tracked[i] || out[2 * i] < 0.f || out[2 * i] >= (float)w || out[2 * i + 1] < 0.f || out[2 * i + 1] >= (float)h) continue;
            cur.push_back({out[2 * i], out[2 * i + 1]});
            prev.push_back({pts[2 * i], pts[2 * i + 1]});
        }
        for (size_t i = 0; i < prev.size(); i += 10) { prev[i].x = (float)((i * 53) % 600 + 20); prev[i].y = (float)((i * 97) % 440 + 20); }
        std::vector<double> grid_device(100, 0.5), grid_host(100, 0.5);          // Frame::Reset_Gridproba
        DSDTM::Rarsac_base on_device(grid_device, cur, prev, w, h, true), on_host(grid_host, cur, prev, w, h, false);
        const std::vector<uint8_t> sd = on_device.RejectFundamental(), sh = on_host.RejectFundamental();
        std::printf("%zu correspondences: device keeps %d (hypothesis %d of %d run), host keeps %d\n", cur.size(), on_device.result.n_inliers,
                    on_device.result.best_hypothesis, on_device.result.iterations_run, on_host.result.n_inliers);
        if (sd != sh || std::memcmp(grid_device.data(), grid_host.data(), 100 * sizeof(double)) != 0 ||
            std::memcmp(on_device.result.F, on_host.result.F, sizeof on_host.result.F) != 0) { std::printf("device and host differ\n"); return 1; }
        std::vector<DSDTM::RarsacPoint2f> kept = cur;
        DSDTM::ReduceFeatures(kept, sd);
        if ((int)kept.size() != on_device.result.n_inliers) { std::printf("ReduceFeatures is wrong\n"); return 1; }
    } catch (const std::exception& e) { std::printf("failed: %s\n", e.what()); return 1; }
    std::printf("ok\n");
    return 0;
}
