// example_motion_ransac.cpp — the whole of Moving_Detecter::Mod_FastMCD (src/Moving_Detection.cpp:19-34) from C++, without OpenCV:
// correspondences -> HomographyEstimator::findHomography (dsdtm_homography_host.hpp, libdsdtm_amd_homography.so) ->
// Moving_Detecter::Mod_FastMCD(..., H, ...) (dsdtm_motion_host.hpp, libdsdtm_amd_motion.so). The frames are synthetic: a textured scene
// that the camera pans over, a bright block that moves on its own, correspondences that follow the pan (with noise) and 30 % outliers.
// A frame for which no homography is found is skipped with a zero mask — where the reference dereferences the empty matrix.
//   build: hipcc example_motion_ransac.cpp -o example_motion_ransac -L../csrc -ldsdtm_amd_motion -ldsdtm_amd_homography -Wl,-rpath,'$ORIGIN/../csrc'
//   usage: example_motion_ransac [frames]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsdtm_homography_host.hpp"
#include "dsdtm_motion_host.hpp"

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 6, W = 640, Hh = 480, pan = 3;
    try {
        dsdtm::HomographyEstimator est(0);
        DSDTM::Moving_Detecter det(0, 480);
        std::vector<uint8_t> img((size_t)W * Hh);
        std::vector<DSDTM::Feature2f> features;
        for (int y = 20; y < Hh; y += 40)
            for (int x = 20; x < W; x += 40) features.push_back({x + 0.5f, y + 0.25f});
        unsigned seed = 7u;
        for (int f = 0; f < frames; ++f) {
            for (int y = 0; y < Hh; ++y)
                for (int x = 0; x < W; ++x) img[(size_t)y * W + x] = (uint8_t)(100 + (((x + pan * f) / 2 * 7 + y / 2 * 13) % 5));
            for (int y = 200; y < 260; ++y)
                for (int x = 100 + 12 * f; x < 180 + 12 * f; ++x) img[(size_t)y * W + x] = 149;
            // tPointsA (this frame) -> tPointsB (the last frame): the scene moved by -pan px in x, so B = A + (pan, 0)
            std::vector<dsdtm::Point2f> A, B;
            for (int i = 0; i < 200; ++i) {
                const float x = 10.0f + (float)(lcg(seed) % 620), y = 10.0f + (float)(lcg(seed) % 460);
                const float nx = ((float)(lcg(seed) % 1000) - 500.0f) / 1000.0f, ny = ((float)(lcg(seed) % 1000) - 500.0f) / 1000.0f;
                A.push_back({x, y});
                if (i % 10 < 3) B.push_back({(float)(lcg(seed) % 640), (float)(lcg(seed) % 480)});
                else B.push_back({x + (float)pan + nx, y + ny});
            }
            double H[9];
            std::vector<uint8_t> inliers;
            dsdtm_homography_result r;
            DSDTM::Mask mask;
            if (!est.findHomography(A, B, H, &inliers, &r)) {
                mask.width = W; mask.height = Hh; mask.data.assign((size_t)W * Hh, 0);
                std::printf("frame %d: no homography, frame skipped with a zero mask\n", f);
                continue;
            }
            det.Mod_FastMCD(img.data(), W, Hh, W, H, features, &mask);
            size_t on = 0;
            for (uint8_t v : mask.data) on += v == 255;
            std::printf("frame %d: %d inliers of %zu, hypothesis %d, %d round(s), %d refit steps, %zu mask pixels, %zu of %zu features kept\n  H =", f,
                        r.n_inliers, A.size(), r.best_hypothesis, r.rounds, r.refit_iterations, on, det.Motion_Removal(features, false).size(), features.size());
            for (int i = 0; i < 9; ++i) std::printf(" %.17g", H[i]);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
