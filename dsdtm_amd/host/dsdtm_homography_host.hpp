// dsdtm_homography_host.hpp — cv::findHomography(ptsA, ptsB, CV_RANSAC) as Moving_Detecter::Mod_FastMCD calls it
// (src/Moving_Detection.cpp:28), over the C ABI of include/dsdtm_amd_homography.h (libdsdtm_amd_homography.so). Header-only; needs
// neither OpenCV nor libdsdtm_amd.so. No CPU compute path: every H comes from the device, a failure throws.
//
//   dsdtm::HomographyEstimator est;                  // one per tracker thread (owns a dsdtm_homography_ctx)
//   double H[9]; std::vector<uint8_t> mask;
//   if (est.findHomography(ptsA, ptsB, H, &mask)) det.Mod_FastMCD(gray, w, h, stride, H, features, &out);      // dsdtm_motion_host.hpp
//
// PARITY: the documented shape of findHomography(..., CV_RANSAC) at its default arguments is kept (4-point samples, forward reprojection
// error against 3 px, confidence 0.995, about 2000 hypotheses at most, a refit on the inliers of the best model, the mask of the RANSAC
// model returned); which samples are drawn, how ties fall, when the loop stops and how the refit iterates are this project's
// definition (see the C header). Parity with OpenCV is unpinned. Where OpenCV returns an empty matrix — which the reference
// dereferences unchecked — findHomography returns false and leaves H and the mask alone: skip the frame.
//
// WHICH PATH. Measured on one MI355X at 200 correspondences with 40 % outliers (profiles/r16_homography.txt): one call for one tracker
// takes 109 us (the kernel 94 us: one workgroup on one compute unit) against 160 us for the plain C implementation of the same
// definition on one host thread — no crossover was found, but a tuned host RANSAC may well be faster than that C program for a SINGLE
// tracker. The batch is what the device is for: findHomographies() for 64 trackers takes 169 us, for 1024 trackers 551 us (0.54 us
// each). A process that runs several trackers should collect their correspondences and make ONE findHomographies call per frame time.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_homography.h"

namespace dsdtm {

struct Point2f { float x, y; };                    // cv::Point2f

class HomographyEstimator {
public:
    explicit HomographyEstimator(int device = 0) {
        if (dsdtm_homography_create(device, &ctx_) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_homography_create: ") + dsdtm_homography_last_error(nullptr));
    }
    ~HomographyEstimator() { dsdtm_homography_destroy(ctx_); }
    HomographyEstimator(const HomographyEstimator&) = delete;
    HomographyEstimator& operator=(const HomographyEstimator&) = delete;

    // One tracker: H (9 doubles, row-major) maps ptsA (current frame) to ptsB (last frame). Returns false — H and mask untouched —
    // with 4 correspondences or fewer (the reference's size() > 4) and where no model was found. `result` receives the counters.
    bool findHomography(const std::vector<Point2f>& ptsA, const std::vector<Point2f>& ptsB, double H[9], std::vector<uint8_t>* mask = nullptr,
                        dsdtm_homography_result* result = nullptr) {
        if (ptsA.size() != ptsB.size()) throw std::runtime_error("findHomography: ptsA and ptsB differ in length");
        std::vector<uint8_t> m(ptsA.size());
        dsdtm_homography_result r;
        r.found = 0;
        check(dsdtm_find_homography(ctx_, (int)ptsA.size(), ptsA.empty() ? nullptr : &ptsA[0].x, ptsB.empty() ? nullptr : &ptsB[0].x,
                                    m.empty() ? nullptr : m.data(), &r), "dsdtm_find_homography");
        if (r.found != 1) return false;
        for (int i = 0; i < 9; ++i) H[i] = r.H[i];
        if (mask) *mask = std::move(m);
        if (result) *result = r;
        return true;
    }

    // n trackers in ONE submission: ptsA[t] -> ptsB[t]. results[t].found tells which H are valid.
    void findHomographies(const std::vector<std::vector<Point2f>>& ptsA, const std::vector<std::vector<Point2f>>& ptsB,
                          std::vector<dsdtm_homography_result>* results, std::vector<std::vector<uint8_t>>* masks = nullptr) {
        if (ptsA.size() != ptsB.size()) throw std::runtime_error("findHomographies: ptsA and ptsB differ in length");
        const size_t n = ptsA.size();
        std::vector<dsdtm_homography_desc> d(n);
        if (masks) masks->assign(n, {});
        for (size_t t = 0; t < n; ++t) {
            if (ptsA[t].size() != ptsB[t].size()) throw std::runtime_error("findHomographies: a tracker's ptsA and ptsB differ in length");
            d[t] = dsdtm_homography_desc{};
            d[t].m = (int32_t)ptsA[t].size();
            d[t].points_a = ptsA[t].empty() ? nullptr : &ptsA[t][0].x;
            d[t].points_b = ptsB[t].empty() ? nullptr : &ptsB[t][0].x;
            if (masks) { (*masks)[t].assign(ptsA[t].size(), 0); d[t].mask = (*masks)[t].empty() ? nullptr : (*masks)[t].data(); }
        }
        results->assign(n, dsdtm_homography_result{});
        check(dsdtm_find_homographies(ctx_, (int)n, d.data(), results->data()), "dsdtm_find_homographies");
    }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_homography_last_error(ctx_));
    }
    dsdtm_homography_ctx* ctx_ = nullptr;
};

}  // namespace dsdtm
