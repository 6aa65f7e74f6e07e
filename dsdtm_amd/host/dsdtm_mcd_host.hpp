// dsdtm_mcd_host.hpp — the contour step of MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:98-128) on the host, and
// Moving_Detecter in the reference's shape over the C ABI of include/dsdtm_amd_mcd.h (libdsdtm_amd_mcd.so). Header-only; needs neither
// OpenCV nor libdsdtm_amd.so.
//
//   DSDTM::BoxResult r = DSDTM::mcd_box_host(mask, w, h, stride, boxed, boxed_stride);      // rules C1-C5, no library needed
//
//   DSDTM::MotionDetector det;                        // one per tracker thread (owns a dsdtm_mcd_ctx)
//   DSDTM::Mask mask;
//   det.Mod_FastMCD(gray, width, height, stride, H, features, &mask);      // the WHOLE MCDWrapper::Run: mask has the rectangle
//   std::vector<DSDTM::Feature2f> rebuilt = det.Motion_Removal(features);
//
// mcd_box_host is bit-equal to dsdtm_amd/contour_restatement.py and to the device (tests/test_mcd_cpu.py, tests/test_mcd_gpu.py). It
// labels by flood fill and walks the border of those components only whose bound 2 (bw - 1)(bh - 1) can still beat the best area2.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_mcd.h"
#include "dsdtm_framediff_host.hpp"
#include "dsdtm_motion_host.hpp"

namespace DSDTM {

struct BoxResult {
    int32_t box[4] = {0, 0, 0, 0};      // x, y, w, h; all 0: nothing drawn
    int64_t area2 = 0;
    int32_t n_components = 0;
    bool operator==(const BoxResult& o) const { return !std::memcmp(box, o.box, sizeof box) && area2 == o.area2 && n_components == o.n_components; }
};

// C1-C5 of include/dsdtm_amd_mcd.h on one mask (rows `stride` apart). boxed: NULL, or where the mask with the rectangle goes (rows
// boxed_stride apart; may be `mask` itself). Throws std::runtime_error if a walk passes its cap of 4 * pixels + 4 steps (it cannot).
inline BoxResult mcd_box_host(const uint8_t* mask, int w, int h, int stride, uint8_t* boxed = nullptr, int boxed_stride = 0) {
    static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    auto on = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && mask[(size_t)y * (size_t)stride + (size_t)x] != 0; };
    std::vector<uint8_t> seen((size_t)w * (size_t)h, 0);
    std::vector<int32_t> stack;
    BoxResult out;
    int best_ext[4] = {0, 0, -1, -1};
    for (int y0 = 0; y0 < h; ++y0)
        for (int x0 = 0; x0 < w; ++x0) {
            if (mask[(size_t)y0 * (size_t)stride + (size_t)x0] == 0 || seen[(size_t)y0 * w + x0]) continue;
            ++out.n_components;
            int minx = x0, maxx = x0, maxy = y0;
            seen[(size_t)y0 * w + x0] = 1;
            stack.assign(1, y0 * w + x0);
            while (!stack.empty()) {
                const int p = stack.back(), cx = p % w, cy = p / w;
                stack.pop_back();
                if (cx < minx) minx = cx;
                if (cx > maxx) maxx = cx;
                if (cy > maxy) maxy = cy;
                for (int k = 0; k < 8; ++k) {
                    const int nx = cx + DX[k], ny = cy + DY[k];
                    if (on(nx, ny) && !seen[(size_t)ny * w + nx]) { seen[(size_t)ny * w + nx] = 1; stack.push_back(ny * w + nx); }
                }
            }
            // components come in raster order of their first pixel, so only a strictly larger area2 wins (C4); it is at most the bound
            if (2 * (int64_t)(maxx - minx) * (maxy - y0) <= out.area2) continue;
            int s = 4;
            do { s = (s - 1) & 7; } while (!on(x0 + DX[s], y0 + DY[s]) && s != 4);
            if (s == 4) continue;
            const int x1 = x0 + DX[s], y1 = y0 + DY[s];
            int x = x0, y = y0;
            int64_t acc = 0, left = 4 * (int64_t)w * h + 4;
            for (;;) {
                if (--left < 0) throw std::runtime_error("mcd_box_host: a contour walk passed its cap of 4 * pixels + 4 steps");
                int nx, ny;
                do { s = (s + 1) & 7; nx = x + DX[s]; ny = y + DY[s]; } while (!on(nx, ny));
                acc += (int64_t)x * ny - (int64_t)y * nx;                              // C3
                if (nx == x0 && ny == y0 && x == x1 && y == y1) break;                 // C2: Suzuki's stop
                x = nx; y = ny; s = (s + 4) & 7;
            }
            if (acc < 0) acc = -acc;
            if (acc > out.area2) { out.area2 = acc; best_ext[0] = minx; best_ext[1] = y0; best_ext[2] = maxx; best_ext[3] = maxy; }
        }
    if (out.area2 > 0) { out.box[0] = best_ext[0]; out.box[1] = best_ext[1]; out.box[2] = best_ext[2] - best_ext[0] + 1; out.box[3] = best_ext[3] - best_ext[1] + 1; }
    if (boxed)
        for (int y = 0; y < h; ++y) {
            if (boxed != mask) std::memcpy(boxed + (size_t)y * (size_t)boxed_stride, mask + (size_t)y * (size_t)stride, (size_t)w);
            if (out.area2 > 0 && y >= best_ext[1] && y <= best_ext[3]) std::memset(boxed + (size_t)y * (size_t)boxed_stride + best_ext[0], 255, (size_t)out.box[2]);      // C5
        }
    return out;
}

// What MotionDetector::Mod_FrameDiff runs on: rules F1-F8 of include/dsdtm_amd_framediff.h for one pair, on the device
// (dsdtm_framediff_step, libdsdtm_amd_framediff.so: link it when on_device is used) or with frame_diff_host; the same bytes either way.
// A class of its own, made by the caller, so that a program that never calls Mod_FrameDiff links what it linked before.
// on_device defaults to true: the device wins everywhere measured, the issue's candidate included (profiles/r25_framediff.txt, 640x480, ONE pair
// from pageable memory with the mask read back: 116 us against 4821 us for frame_diff_host on one thread, this repository's C++, not OpenCV).
#ifndef FRAMEDIFF_ON_DEVICE_DEFAULT
#define FRAMEDIFF_ON_DEVICE_DEFAULT true
#endif
class FrameDiffer {
public:
    explicit FrameDiffer(int device = 0, bool on_device = FRAMEDIFF_ON_DEVICE_DEFAULT) : on_device_(on_device) {
        if (on_device_ && dsdtm_framediff_create(device, &ctx_) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_framediff_create: ") + dsdtm_framediff_last_error(nullptr));
    }
    ~FrameDiffer() { if (ctx_) dsdtm_framediff_destroy(ctx_); }
    FrameDiffer(const FrameDiffer&) = delete;
    FrameDiffer& operator=(const FrameDiffer&) = delete;
    // mask: width x height bytes, packed. Throws where the entry refuses.
    dsdtm_framediff_result run(const uint8_t* a, int a_stride, const uint8_t* b, int b_stride, int width, int height, const double H[9], int flags,
                               int threshold, int maxval, uint8_t* mask, int n_features, const float* feature_px, uint8_t* feature_on_mask) {
        dsdtm_framediff_result r{};
        if (on_device_) {
            dsdtm_framediff_desc d{};
            d.a = a; d.b = b; d.width = width; d.height = height; d.a_stride = a_stride; d.b_stride = b_stride;
            std::memcpy(d.H, H, sizeof d.H);
            d.flags = flags; d.threshold = threshold; d.maxval = maxval; d.mask = mask; d.mask_stride = width;
            d.n_features = n_features; d.feature_px = feature_px; d.feature_on_mask = feature_on_mask;
            if (dsdtm_framediff_step(ctx_, &d, &r) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_framediff_step: ") + dsdtm_framediff_last_error(ctx_));
            return r;
        }
        for (int i = 0; i < n_features; ++i) {          // (the entry's refusal; frame_diff_host takes the features on trust)
            const float x = std::nearbyintf(feature_px[2 * (size_t)i]), y = std::nearbyintf(feature_px[2 * (size_t)i + 1]);
            if (!(x >= 0 && x < (float)width && y >= 0 && y < (float)height)) throw std::runtime_error("frame_diff_host: a feature rounds outside the image");
        }
        const FrameDiffHost h = frame_diff_host(a, a_stride, b, b_stride, width, height, H, flags, threshold, maxval, mask, width, n_features, feature_px, feature_on_mask);
        if (!h.ok) throw std::runtime_error("frame_diff_host: H is singular or not finite");
        std::memcpy(r.M, h.M, sizeof r.M);
        r.n_foreground = h.n_foreground; r.n_flagged = h.n_flagged;
        return r;
    }
    bool on_device() const { return on_device_; }

private:
    dsdtm_framediff_ctx* ctx_ = nullptr;
    bool on_device_ = true;
};

// Moving_Detecter (src/Moving_Detection.cpp) + Frame::Motion_Removal (src/Frame.cpp:342-363) with Mod_FastMCD = the WHOLE
// MCDWrapper::Run. Two paths, the same bytes; link both libraries (each path creates the context of its own library only):
//   host_box = true, the default and for ONE tracker the faster path (profiles/r23_mcd.txt: 346 us against 1039 us at 640x480):
//     dsdtm_motion_step (libdsdtm_amd_motion.so) returns detect_img, then mcd_box_host and the lookup of C6 run here;
//   host_box = false: one dsdtm_mcd_step (libdsdtm_amd_mcd.so) — contour step, fill and lookup on the device, one submission.
// Many trackers belong in one dsdtm_mcd_steps call (17 us per model at n = 1024 against 365 us on the host path).
class MotionDetector {
public:
    explicit MotionDetector(int device = 0, int required_rows = 0, bool host_box = true) : required_rows_(required_rows), host_box_(host_box) {
        if (host_box_) {
            if (dsdtm_motion_create(device, &mctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_motion_create: ") + dsdtm_motion_last_error(nullptr));
        } else if (dsdtm_mcd_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_mcd_create: ") + dsdtm_mcd_last_error(nullptr));
    }
    ~MotionDetector() {
        if (host_box_) { if (mmodel_) dsdtm_motion_model_destroy(mctx_, mmodel_); dsdtm_motion_destroy(mctx_); }
        else { if (model_) dsdtm_mcd_model_destroy(ctx_, model_); dsdtm_mcd_destroy(ctx_); }
    }
    MotionDetector(const MotionDetector&) = delete;
    MotionDetector& operator=(const MotionDetector&) = delete;

    // Returns false — nothing done — for an image of another height than required_rows, as Tracking::MotionRemoval does (src/Tracking.cpp:509).
    bool Mod_FastMCD(const uint8_t* gray, int width, int height, int stride, const double H[9], const std::vector<Feature2f>& features, Mask* out) {
        if (required_rows_ && height != required_rows_) return false;
        Mask m;
        m.width = width; m.height = height; m.data.assign((size_t)width * (size_t)height, 0);
        on_mask_.assign(features.size(), 0);
        const float* px = features.empty() ? nullptr : &features[0].x;
        uint8_t* flags = features.empty() ? nullptr : on_mask_.data();
        if (!host_box_) {
            if (!model_) check(dsdtm_mcd_model_create(ctx_, width, height, &model_), "dsdtm_mcd_model_create");
            check(dsdtm_mcd_step(ctx_, model_, gray, stride, H, nullptr, 0, m.data.data(), width, (int)features.size(), px, flags,
                                 last_.box, &last_.area2, &last_.n_components), "dsdtm_mcd_step");
        } else {
            if (!mmodel_) check(dsdtm_motion_model_create(mctx_, width, height, &mmodel_), "dsdtm_motion_model_create");
            // (the flags it returns are detect_img's and are overwritten below; asking for them makes the entry check every feature)
            check(dsdtm_motion_step(mctx_, mmodel_, gray, stride, H, m.data.data(), width, (int)features.size(), px, flags), "dsdtm_motion_step");
            last_ = mcd_box_host(m.data.data(), width, height, width, m.data.data(), width);
            for (size_t i = 0; i < features.size(); ++i)        // C6
                on_mask_[i] = m.data[(size_t)std::nearbyintf(features[i].y) * (size_t)width + (size_t)std::nearbyintf(features[i].x)] == 255;
        }
        if (out) *out = std::move(m);
        return true;
    }
    // The same without an H argument, as MCDWrapper::Run works: `klt` (a DSDTM::KLTWrapper of dsdtm_klt_host.hpp, which the caller owns and
    // includes) tracks its grid from the last image into this one and its H goes into the step above. The first image seeds it (identity).
    template <class Klt>
    bool Mod_FastMCD_KLT(const uint8_t* gray, int width, int height, int stride, Klt& klt, const std::vector<Feature2f>& features, Mask* out) {
        if (required_rows_ && height != required_rows_) return false;
        klt.RunTrack(gray, width, height, stride);
        double H[9];
        klt.GetHomography(H);
        return Mod_FastMCD(gray, width, height, stride, (const double*)H, features, out);
    }
    // Moving_Detecter::Mod_FrameDiff (src/Moving_Detection.cpp:36-63) behind its findHomography: H is the caller's (a HomographyEstimator's
    // fit of frame B's points onto frame A's, or a KLTWrapper's with DSDTM_FRAMEDIFF_INVERSE_MAP in `flags`), `differ` a FrameDiffer the
    // caller owns. gray_b IS FRAME B: the reference's :45 passes frame A twice (QUIRK 1 of include/dsdtm_amd_framediff.h); a caller who
    // wants that passes gray_a for both. maxval 0 is the reference's 200, at which Motion_Removal removes nothing (QUIRK 2); 255 makes
    // the mask act. Returns false — nothing done — with fewer than 4 points (:40-41).
    template <class Differ>
    bool Mod_FrameDiff(Differ& differ, const uint8_t* gray_a, const uint8_t* gray_b, int width, int height, int stride, size_t n_points, const double H[9],
                       const std::vector<Feature2f>& features, Mask* out, int flags = 0, int threshold = DSDTM_FRAMEDIFF_THRESHOLD, int maxval = 0) {
        if (n_points < 4) return false;
        Mask m;
        m.width = width; m.height = height; m.data.assign((size_t)width * (size_t)height, 0);
        on_mask_.assign(features.size(), 0);
        last_framediff_ = differ.run(gray_a, stride, gray_b, stride, width, height, H, flags, threshold, maxval, m.data.data(), (int)features.size(),
                                     features.empty() ? nullptr : &features[0].x, features.empty() ? nullptr : on_mask_.data());
        if (out) *out = std::move(m);
        return true;
    }
    const dsdtm_framediff_result& framediff() const { return last_framediff_; }
    std::vector<Feature2f> Motion_Removal(const std::vector<Feature2f>& features, bool faithful = true) const {
        if (features.size() != on_mask_.size()) throw std::runtime_error("Motion_Removal: not the features the last Mod_FastMCD was given");
        std::vector<Feature2f> out;
        if (faithful) out = features;
        for (size_t i = 0; i < features.size(); ++i) if (!on_mask_[i]) out.push_back(features[i]);
        return out;
    }
    const std::vector<uint8_t>& on_mask() const { return on_mask_; }
    const BoxResult& box() const { return last_; }
    void Reset() {
        if (model_) check(dsdtm_mcd_model_reset(ctx_, model_), "dsdtm_mcd_model_reset");
        if (mmodel_) check(dsdtm_motion_model_reset(mctx_, mmodel_), "dsdtm_motion_model_reset");
    }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + (host_box_ ? dsdtm_motion_last_error(mctx_) : dsdtm_mcd_last_error(ctx_)));
    }
    dsdtm_mcd_ctx* ctx_ = nullptr;
    dsdtm_mcd_model* model_ = nullptr;
    dsdtm_motion_ctx* mctx_ = nullptr;
    dsdtm_motion_model* mmodel_ = nullptr;
    int required_rows_ = 0;
    bool host_box_ = true;
    BoxResult last_;
    dsdtm_framediff_result last_framediff_{};
    std::vector<uint8_t> on_mask_;
};

}  // namespace DSDTM
