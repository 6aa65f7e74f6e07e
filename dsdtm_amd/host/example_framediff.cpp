// example_framediff.cpp — Moving_Detecter::Mod_FrameDiff without OpenCV: DSDTM::MotionDetector::Mod_FrameDiff (dsdtm_mcd_host.hpp) over
// libdsdtm_amd_framediff.so, on the device and with frame_diff_host, the same bytes.
//
//   g++ -O2 -std=c++14 -ffp-contract=off example_framediff.cpp ../csrc/libdsdtm_amd_framediff.so ../csrc/libdsdtm_amd_mcd.so ../csrc/libdsdtm_amd_motion.so
//       -Wl,-rpath,../csrc -L/opt/rocm/lib -lamdhip64 -o example_framediff
//
// A smooth scene moves 3 pixels to the right between frame B and frame A and a bright block appears in frame A. H is the translation by
// 3 (frame B's points onto frame A's). The program exits with 0 only when the device's mask equals the host function's in every byte,
// the features on the block are flagged at maxval 255 and none is at the reference's 200 (QUIRK 2 of include/dsdtm_amd_framediff.h).
#include <cmath>
#include <cstdio>
#include <vector>

#include "dsdtm_mcd_host.hpp"

static std::vector<uint8_t> frame(int w, int h, int shift, bool block) {
    std::vector<uint8_t> g((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double u = x - shift;
            double v = 110.0 + 40.0 * std::sin(u * 0.21 + y * 0.05) + 35.0 * std::cos(y * 0.17 - u * 0.07);
            if (block && x >= 140 && x < 200 && y >= 90 && y < 150) v = 255.0;
            g[(size_t)y * w + x] = (uint8_t)v;
        }
    return g;
}

int main() {
    const int w = 320, h = 240;
    try {
        const std::vector<uint8_t> b = frame(w, h, 0, false), a = frame(w, h, 3, true);
        const double H[9] = {1, 0, 3, 0, 1, 0, 0, 0, 1};
        const std::vector<DSDTM::Feature2f> features{{170.f, 120.f}, {150.5f, 100.5f}, {40.f, 40.f}, {300.f, 200.f}};
        DSDTM::MotionDetector det(0, 0, false);
        DSDTM::FrameDiffer device(0, true), host(0, false);
        DSDTM::Mask md, mh, m200;
        if (!det.Mod_FrameDiff(device, a.data(), b.data(), w, h, w, 8, H, features, &md, 0, DSDTM_FRAMEDIFF_THRESHOLD, 255)) return 1;
        const std::vector<uint8_t> on_device = det.on_mask();
        const dsdtm_framediff_result rd = det.framediff();
        if (!det.Mod_FrameDiff(host, a.data(), b.data(), w, h, w, 8, H, features, &mh, 0, DSDTM_FRAMEDIFF_THRESHOLD, 255)) return 1;
        const dsdtm_framediff_result rh = det.framediff();
        std::printf("device: %d foreground pixels, %d flagged; host: %d, %d\n", rd.n_foreground, rd.n_flagged, rh.n_foreground, rh.n_flagged);
        if (md.data != mh.data || on_device != det.on_mask() || std::memcmp(&rd, &rh, sizeof rd) != 0) { std::printf("device and host differ\n"); return 1; }
        if (on_device != std::vector<uint8_t>{1, 1, 0, 0} || det.Motion_Removal(features, false).size() != 2) { std::printf("flags are wrong\n"); return 1; }
        if (!det.Mod_FrameDiff(device, a.data(), b.data(), w, h, w, 8, H, features, &m200)) return 1;
        if (det.framediff().n_flagged != 0 || det.framediff().n_foreground != rd.n_foreground || det.Motion_Removal(features, false).size() != 4) return 1;
        if (det.Mod_FrameDiff(device, a.data(), b.data(), w, h, w, 3, H, features, &m200)) return 1;          // fewer than 4 points
    } catch (const std::exception& e) { std::printf("failed: %s\n", e.what()); return 1; }
    std::printf("ok\n");
    return 0;
}
