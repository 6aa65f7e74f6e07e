// example_motion.cpp — a C++ caller of libdsdtm_amd_motion.so through dsdtm_motion_host.hpp, in the shape of
// Tracking::MotionRemoval (src/Tracking.cpp:487-512): per frame one Mod_FastMCD with the homography the caller estimated, then
// Motion_Removal over the frame's features. Here the frames are synthetic (a flat textured scene, a bright block that moves) and the
// homography is the identity; a real caller passes cv::findHomography(tPointsA, tPointsB, CV_RANSAC).
//   build: hipcc example_motion.cpp -o example_motion -L../csrc -ldsdtm_amd_motion -Wl,-rpath,'$ORIGIN/../csrc'
//   usage: example_motion [frames]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsdtm_motion_host.hpp"

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 6, W = 640, Hh = 480;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    try {
        DSDTM::Moving_Detecter det(0, 480);
        std::vector<uint8_t> img((size_t)W * Hh);
        std::vector<DSDTM::Feature2f> features;
        for (int y = 20; y < Hh; y += 40)
            for (int x = 20; x < W; x += 40) features.push_back({x + 0.5f, y + 0.25f});
        for (int f = 0; f < frames; ++f) {
            for (int y = 0; y < Hh; ++y)
                for (int x = 0; x < W; ++x) img[(size_t)y * W + x] = (uint8_t)(100 + ((x / 2 * 7 + y / 2 * 13) % 5));
            for (int y = 200; y < 260; ++y)
                for (int x = 100 + 12 * f; x < 180 + 12 * f; ++x) img[(size_t)y * W + x] = 149;
            DSDTM::Mask mask;
            det.Mod_FastMCD(img.data(), W, Hh, W, I, features, &mask);
            size_t on = 0;
            for (uint8_t v : mask.data) on += v == 255;
            const size_t kept = det.Motion_Removal(features, false).size();
            std::printf("frame %d: %zu mask pixels, %zu of %zu features kept (the reference's list would hold %zu)\n", f, on, kept,
                        features.size(), det.Motion_Removal(features).size());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
