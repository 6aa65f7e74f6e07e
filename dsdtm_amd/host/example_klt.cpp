// example_klt.cpp — images -> H -> boxed mask without OpenCV and without a map: DSDTM::KLTWrapper (dsdtm_klt_host.hpp, libdsdtm_amd_klt.so)
// in front of DSDTM::MotionDetector (dsdtm_mcd_host.hpp, libdsdtm_amd_mcd.so / libdsdtm_amd_motion.so).
//
//   g++ -O2 -std=c++14 -ffp-contract=off example_klt.cpp ../csrc/libdsdtm_amd_klt.so ../csrc/libdsdtm_amd_mcd.so ../csrc/libdsdtm_amd_motion.so
//       -Wl,-rpath,../csrc -L/opt/rocm/lib -lamdhip64 -o example_klt
//
// A smooth synthetic scene moves 3 pixels to the right per frame. The program exits with 0 only when every RunTrack after the first
// comes from the RANSAC, its H is the translation by -3 (current -> previous) to within 0.05 px, and the device's points equal
// klt_step_host's survivors in number.
#include <cmath>
#include <cstdio>
#include <vector>

#include "dsdtm_klt_host.hpp"
#include "dsdtm_mcd_host.hpp"

static std::vector<uint8_t> frame(int w, int h, int shift) {
    std::vector<uint8_t> g((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double u = x - shift;
            g[(size_t)y * w + x] = (uint8_t)(128.0 + 45.0 * std::sin(u * 0.21 + y * 0.05) + 40.0 * std::cos(y * 0.17 - u * 0.07) + 30.0 * std::sin(u * 0.09) * std::cos(y * 0.11));
        }
    return g;
}

int main() {
    const int w = 320, h = 240;
    try {
        DSDTM::KLTWrapper klt;
        DSDTM::MotionDetector det;
        const std::vector<DSDTM::Feature2f> features{{100.f, 100.f}, {200.f, 50.f}};
        std::vector<uint8_t> last;
        for (int k = 0; k < 4; ++k) {
            const std::vector<uint8_t> g = frame(w, h, 3 * k);
            DSDTM::Mask mask;
            if (!det.Mod_FastMCD_KLT(g.data(), w, h, w, klt, features, &mask)) { std::printf("Mod_FastMCD refused frame %d\n", k); return 1; }
            const dsdtm_klt_result& r = klt.last();
            std::printf("frame %d: source %d, %d of %d tracked, %d inliers, H = [%.4f %.4f %.4f; %.4f %.4f %.4f]\n", k, r.source, r.n_tracked, r.n_points,
                        r.n_inliers, r.H[0], r.H[1], r.H[2], r.H[3], r.H[4], r.H[5]);
            if (k == 0) { if (r.source != DSDTM_KLT_SOURCE_IDENTITY || r.n_tracked != 0) return 1; }
            else {
                if (r.source != DSDTM_KLT_SOURCE_RANSAC || std::fabs(r.H[2] + 3.0) > 0.05 || std::fabs(r.H[5]) > 0.05 || std::fabs(r.H[0] - 1.0) > 1e-3) return 1;
                std::vector<std::vector<uint8_t>> s0, s1;
                const std::vector<DSDTM::KltLevel> p0 = DSDTM::klt_pyramid_host(last.data(), w, h, w, 4, s0), p1 = DSDTM::klt_pyramid_host(g.data(), w, h, w, 4, s1);
                const DSDTM::KltStepHost hs = DSDTM::klt_step_host(p0.data(), p1.data(), 4);
                if (hs.n_tracked != r.n_tracked || hs.n_points != r.n_points) { std::printf("host tracks %d of %d\n", hs.n_tracked, hs.n_points); return 1; }
            }
            last = g;
        }
    } catch (const std::exception& e) { std::printf("failed: %s\n", e.what()); return 1; }
    std::printf("ok\n");
    return 0;
}
