// dsdtm_motion_host.hpp — Moving_Detecter (src/Moving_Detection.cpp) and Frame::Motion_Removal (src/Frame.cpp:342-363) in the
// reference's shape, over the C ABI of include/dsdtm_amd_motion.h (libdsdtm_amd_motion.so). Header-only; needs neither OpenCV nor
// libdsdtm_amd.so. No CPU compute path: every mask comes from the device, a failure throws.
//
//   DSDTM::Moving_Detecter det;                       // one per tracker thread (owns a dsdtm_motion_ctx)
//   DSDTM::Mask mask;
//   det.Mod_FastMCD(gray, width, height, stride, H, features, &mask);      // H: cv::findHomography(tPointsA, tPointsB, CV_RANSAC)
//   std::vector<DSDTM::Feature2f> rebuilt = det.Motion_Removal(features);
//
// Mod_FastMCD is MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137) up to BGModel.update(detect_img): the mask BEFORE
// the contour step (:98-128), which is out of scope (see the C header). The model is created on the first image (frm_cnt == 0, :67).
// Tracking::MotionRemoval returns early unless the image has 480 rows (src/Tracking.cpp:509): here `required_rows` (0: no such
// test). The reference's call of MotionRemoval is commented out (src/Tracking.cpp:230).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_motion.h"

namespace DSDTM {

struct Feature2f { float x, y; };                  // Feature::mpx (include/Feature.h)
struct Mask {                                      // cv::Mat CV_8UC1, 255 / 0
    int width = 0, height = 0;
    std::vector<uint8_t> data;
    uint8_t at(int x, int y) const { return data[(size_t)y * (size_t)width + (size_t)x]; }
};

class Moving_Detecter {
public:
    explicit Moving_Detecter(int device = 0, int required_rows = 0) : required_rows_(required_rows) {
        if (dsdtm_motion_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_motion_create: ") + dsdtm_motion_last_error(nullptr));
    }
    ~Moving_Detecter() {
        if (model_) dsdtm_motion_model_destroy(ctx_, model_);
        dsdtm_motion_destroy(ctx_);
    }
    Moving_Detecter(const Moving_Detecter&) = delete;
    Moving_Detecter& operator=(const Moving_Detecter&) = delete;

    // `gray` in host memory or in this device's memory (read where it is). `features`: those of the current frame; their flags come
    // back from the same submission (Motion_Removal below). Returns false — nothing done — for an image of another height than
    // required_rows, as Tracking::MotionRemoval does.
    bool Mod_FastMCD(const uint8_t* gray, int width, int height, int stride, const double H[9], const std::vector<Feature2f>& features, Mask* out) {
        if (required_rows_ && height != required_rows_) return false;
        if (!model_) check(dsdtm_motion_model_create(ctx_, width, height, &model_), "dsdtm_motion_model_create");
        width_ = width; height_ = height;
        Mask m;
        m.width = width; m.height = height; m.data.assign((size_t)width * (size_t)height, 0);
        on_mask_.assign(features.size(), 0);
        check(dsdtm_motion_step(ctx_, model_, gray, stride, H, m.data.data(), width, (int)features.size(),
                                features.empty() ? nullptr : &features[0].x, features.empty() ? nullptr : on_mask_.data()), "dsdtm_motion_step");
        if (out) *out = std::move(m);
        return true;
    }
    // Frame::Motion_Removal (src/Frame.cpp:342-363) with the flags of the last Mod_FastMCD (feature i lies on the mask when the mask at
    // (cvRound(x), cvRound(y)) is 255, :352). What the reference ends with is NOT the filtered list: tmpFeatures starts as a COPY of all
    // features and the kept ones are appended again (:346-356). `faithful` = true returns that list; false returns the kept ones only.
    std::vector<Feature2f> Motion_Removal(const std::vector<Feature2f>& features, bool faithful = true) const {
        if (features.size() != on_mask_.size()) throw std::runtime_error("Motion_Removal: not the features the last Mod_FastMCD was given");
        std::vector<Feature2f> out;
        if (faithful) out = features;
        for (size_t i = 0; i < features.size(); ++i) if (!on_mask_[i]) out.push_back(features[i]);
        return out;
    }
    const std::vector<uint8_t>& on_mask() const { return on_mask_; }
    void Reset() { if (model_) check(dsdtm_motion_model_reset(ctx_, model_), "dsdtm_motion_model_reset"); }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_motion_last_error(ctx_));
    }
    dsdtm_motion_ctx* ctx_ = nullptr;
    dsdtm_motion_model* model_ = nullptr;
    int required_rows_ = 0, width_ = 0, height_ = 0;
    std::vector<uint8_t> on_mask_;
};

}  // namespace DSDTM
