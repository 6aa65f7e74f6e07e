// libdsdtm_amd_mcd.so's host side (dsdtm_amd/csrc/mcd_api.cpp over motion_api_body.h) against the fake HIP runtime of tests/fake_hip
// (unmodified): the packing of n whole MCDWrapper::Run steps and of n masks into one block, every copy, launch and wait of the new
// entries failing once — all or nothing each time — and the argument checks, as a stand-alone program under ASan/UBSan/LSan. The
// launches are the fakes of tests/fake_hip_motion/fake_motion.cpp and tests/fake_hip_mcd/fake_contour.cpp.
// Test infrastructure (tests/test_mcd_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_mcd_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_contour.h"
#include "fake_hip.h"
#include "fake_motion.h"

static const double IDENT[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

// a bright block, a smaller one and dots: the fake step's detect_img is image >= 128
static void paint(std::vector<uint8_t>& img, int w, int h, int stride) {
    for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)(i % 97);
    for (int y = h / 4; y < h / 2; ++y) for (int x = w / 4; x < w / 2 + 3; ++x) img[(size_t)y * stride + x] = 200;
    for (int y = h - 5; y < h - 2; ++y) for (int x = 2; x < 6; ++x) img[(size_t)y * stride + x] = 255;
    for (int k = 0; k < 9; ++k) img[(size_t)((k * 5) % h) * stride + (size_t)((k * 11) % w)] = 130;
}

// one model's whole Run: outputs prefilled with 0xA5
struct Step {
    int w = 0, h = 0, stride = 0, nf = 0;
    dsdtm_mcd_model* model = nullptr;
    std::vector<uint8_t> img, mask, raw, flags;
    std::vector<float> feat;
    uint8_t* dev_img = nullptr;
    double H[9];
    dsdtm_mcd_desc d{};
    bool init(dsdtm_mcd_ctx* ctx, int w_, int h_, int stride_, int nf_, bool device_image, bool want_mask = true, bool want_raw = true) {
        w = w_; h = h_; stride = stride_; nf = nf_;
        memcpy(H, IDENT, sizeof H);
        CHECK(dsdtm_mcd_model_create(ctx, w, h, &model) == DSDTM_OK && model);
        img.resize((size_t)stride * h);
        paint(img, w, h, stride);
        if (device_image) {
            CHECK(hipMalloc((void**)&dev_img, img.size()) == hipSuccess);
            memcpy(dev_img, img.data(), img.size());
        }
        mask.resize(want_mask ? (size_t)(w + 3) * h : 0);
        raw.resize(want_raw ? (size_t)(w + 1) * h : 0);
        flags.resize((size_t)nf);
        feat.resize(2 * (size_t)nf);
        for (int f = 0; f < nf; ++f) { feat[2 * f] = (float)((f * 7) % w) + 0.25f; feat[2 * f + 1] = (float)((f * 5) % (h - 1)) + 0.5f * (f % 2); }
        d.model = model; d.image = device_image ? dev_img : img.data(); d.stride = stride; d.H = H;
        d.mask = want_mask ? mask.data() : nullptr; d.mask_stride = w + 3;
        d.mask_raw = want_raw ? raw.data() : nullptr; d.mask_raw_stride = w + 1;
        d.n_features = nf; d.feature_px = nf ? feat.data() : nullptr; d.feature_on_mask = nf ? flags.data() : nullptr;
        prefill();
        return true;
    }
    void prefill() {
        fill_a5(mask.data(), mask.size()); fill_a5(raw.data(), raw.size()); fill_a5(flags.data(), flags.size());
        fill_a5(d.box, sizeof d.box); fill_a5(&d.area2, sizeof d.area2); fill_a5(&d.n_components, sizeof d.n_components);
    }
    bool untouched() const {
        return all_a5(mask.data(), mask.size()) && all_a5(raw.data(), raw.size()) && all_a5(flags.data(), flags.size()) && all_a5(d.box, sizeof d.box) &&
               all_a5(&d.area2, sizeof d.area2) && all_a5(&d.n_components, sizeof d.n_components);
    }
    bool answered() const {          // what the fake launches leave: detect_img = image >= 128, then mcd_box_host on it
        std::vector<uint8_t> det((size_t)w * h), boxed((size_t)w * h);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) det[(size_t)y * w + x] = img[(size_t)y * stride + x] >= 128 ? 255 : 0;
        const DSDTM::BoxResult want = DSDTM::mcd_box_host(det.data(), w, h, w, boxed.data(), w);
        CHECK(want.area2 > 0 && want.n_components >= 2);
        CHECK(!memcmp(d.box, want.box, sizeof want.box) && d.area2 == want.area2 && d.n_components == want.n_components);
        for (int y = 0; y < h; ++y) {
            if (!mask.empty()) for (int x = 0; x < w + 3; ++x) CHECK(mask[(size_t)y * (w + 3) + x] == (x < w ? boxed[(size_t)y * w + x] : 0xA5));
            if (!raw.empty()) for (int x = 0; x < w + 1; ++x) CHECK(raw[(size_t)y * (w + 1) + x] == (x < w ? det[(size_t)y * w + x] : 0xA5));
        }
        for (int f = 0; f < nf; ++f) CHECK(flags[f] == (boxed[(size_t)nearbyintf(feat[2 * f + 1]) * w + (size_t)nearbyintf(feat[2 * f])] == 255 ? 1 : 0));
        return true;
    }
    // the fake step writes src + 1 everywhere: the model's generation count
    bool generation(dsdtm_mcd_ctx* ctx, float want) const {
        std::vector<float> st(12 * (size_t)(w / 4) * (size_t)(h / 4), -1.0f);
        CHECK(dsdtm_mcd_model_read(ctx, model, st.data()) == DSDTM_OK);
        for (float v : st) CHECK(v == want);
        return true;
    }
    void release(dsdtm_mcd_ctx* ctx) {
        dsdtm_mcd_model_destroy(ctx, model); model = nullptr;
        if (dev_img) (void)hipFree(dev_img);
        dev_img = nullptr;
    }
};

static int run(dsdtm_mcd_ctx* ctx, std::vector<Step>& s) {
    std::vector<dsdtm_mcd_desc> d;
    for (auto& x : s) d.push_back(x.d);
    const int rc = dsdtm_mcd_steps(ctx, (int)d.size(), d.data());
    for (size_t k = 0; k < s.size(); ++k) s[k].d = d[k];
    return rc;
}

// every copy, launch and wait of dsdtm_mcd_steps failing once: an error, the outputs (the descs' fields included) and the models'
// generations untouched, nothing pending, nothing leaked; the next call succeeds
static bool step_failures() {
    dsdtm_mcd_ctx* ctx = nullptr;
    CHECK(dsdtm_mcd_create(0, &ctx) == DSDTM_OK);
    std::vector<Step> s(3);
    CHECK(s[0].init(ctx, 64, 48, 64, 20, false) && s[1].init(ctx, 70, 50, 80, 0, true) && s[2].init(ctx, 33, 17, 40, 5, false, false, false));
    float gen = 1.0f;
    CHECK(run(ctx, s) == DSDTM_OK);
    gen += 1.0f;
    for (auto& x : s) { CHECK(x.answered() && x.generation(ctx, gen)); x.prefill(); }
    const size_t live0 = fake_hip_live_allocations();
    auto failed_cleanly = [&](int rc) {
        CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_mcd_last_error(ctx)) > 0);
        for (auto& x : s) CHECK(x.untouched() && x.generation(ctx, gen));
        CHECK(run(ctx, s) == DSDTM_OK);
        gen += 1.0f;
        for (auto& x : s) { CHECK(x.answered() && x.generation(ctx, gen)); x.prefill(); }
        return true;
    };
    const long c0 = fake_hip_calls("hipMemcpyAsync"), y0 = fake_hip_calls("hipStreamSynchronize");
    CHECK(run(ctx, s) == DSDTM_OK);
    gen += 1.0f;
    for (auto& x : s) { CHECK(x.answered()); x.prefill(); }
    // one submission: the upload, detect_img, the flags and results, the images with the rectangle; the four launches' drains and the wait
    const long copies = fake_hip_calls("hipMemcpyAsync") - c0, waits = fake_hip_calls("hipStreamSynchronize") - y0;
    CHECK(copies == 4 && waits == 5);
    for (long nth = 1; nth <= copies; ++nth) {
        fake_hip_fail("hipMemcpyAsync", nth);
        const int rc = run(ctx, s);
        fake_hip_fail("hipMemcpyAsync", 0);
        CHECK(failed_cleanly(rc));
    }
    for (long nth = 1; nth <= waits; ++nth) {
        fake_hip_fail("hipStreamSynchronize", nth);
        const int rc = run(ctx, s);
        fake_hip_fail("hipStreamSynchronize", 0);
        CHECK(failed_cleanly(rc));
    }
    for (long nth = 1; nth <= 2; ++nth) {                   // the step launch, the feature lookup
        fake_motion_fail(nth);
        const int rc = run(ctx, s);
        fake_motion_fail(0);
        CHECK(failed_cleanly(rc));
    }
    for (long nth = 1; nth <= 2; ++nth) {                   // the contour launches, the fill
        fake_contour_fail(nth);
        const int rc = run(ctx, s);
        fake_contour_fail(0);
        CHECK(failed_cleanly(rc));
    }
    // the single entry is the batch entry with n = 1
    int32_t box[4]; int64_t area2 = -5; int32_t count = -5;
    fill_a5(box, sizeof box);
    Step& a = s[0];
    fake_contour_fail(1);
    CHECK(dsdtm_mcd_step(ctx, a.model, a.d.image, 64, IDENT, a.raw.data(), 65, a.mask.data(), 67, 20, a.feat.data(), a.flags.data(), box, &area2, &count) == DSDTM_ERR_HIP);
    fake_contour_fail(0);
    CHECK(a.untouched() && all_a5(box, sizeof box) && area2 == -5 && count == -5 && a.generation(ctx, gen));
    CHECK(dsdtm_mcd_step(ctx, a.model, a.d.image, 64, IDENT, a.raw.data(), 65, a.mask.data(), 67, 20, a.feat.data(), a.flags.data(), box, &area2, &count) == DSDTM_OK);
    memcpy(a.d.box, box, sizeof box); a.d.area2 = area2; a.d.n_components = count;
    CHECK(a.answered() && a.generation(ctx, gen + 1.0f) && s[1].generation(ctx, gen));
    a.prefill();
    CHECK(dsdtm_mcd_step(ctx, a.model, a.d.image, 64, IDENT, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == DSDTM_OK && a.untouched());
    CHECK(fake_hip_live_allocations() == live0);
    // a fresh context whose staging block cannot be had: pinned, then device
    for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
        dsdtm_mcd_ctx* c2 = nullptr;
        CHECK(dsdtm_mcd_create(0, &c2) == DSDTM_OK);
        std::vector<Step> q(1);
        CHECK(q[0].init(c2, 64, 48, 64, 9, false));
        for (long nth = 1; nth <= 2; ++nth) {
            fake_hip_fail(api, nth);
            const int rc = run(c2, q);
            fake_hip_fail(api, 0);
            if (rc == DSDTM_OK) { CHECK(q[0].answered()); q[0].prefill(); continue; }      // (fewer than nth calls of this api)
            CHECK(rc == DSDTM_ERR_HIP && q[0].untouched() && fake_hip_pending() == 0);
            CHECK(run(c2, q) == DSDTM_OK && q[0].answered());
            q[0].prefill();
        }
        q[0].release(c2);
        dsdtm_mcd_destroy(c2);
    }
    for (auto& x : s) x.release(ctx);
    dsdtm_mcd_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// dsdtm_mcd_boxes: masks in host and in "device" memory, with strides
struct Box {
    int w = 0, h = 0, stride = 0;
    std::vector<uint8_t> m, boxed;
    uint8_t* dev = nullptr;
    dsdtm_mcd_box_desc d{};
    bool init(int w_, int h_, int stride_, bool device, bool want_boxed) {
        w = w_; h = h_; stride = stride_;
        m.resize((size_t)stride * h);
        paint(m, w, h, stride);
        for (auto& v : m) v = v >= 128 ? v : 0;
        if (device) { CHECK(hipMalloc((void**)&dev, m.size()) == hipSuccess); memcpy(dev, m.data(), m.size()); }
        boxed.resize(want_boxed ? (size_t)(w + 2) * h : 0);
        d.mask = device ? dev : m.data(); d.width = w; d.height = h; d.stride = stride;
        d.boxed = want_boxed ? boxed.data() : nullptr; d.boxed_stride = w + 2;
        prefill();
        return true;
    }
    void prefill() { fill_a5(boxed.data(), boxed.size()); fill_a5(d.box, sizeof d.box); fill_a5(&d.area2, 8); fill_a5(&d.n_components, 4); }
    bool untouched() const { return all_a5(boxed.data(), boxed.size()) && all_a5(d.box, sizeof d.box) && all_a5(&d.area2, 8) && all_a5(&d.n_components, 4); }
    bool answered() const {
        std::vector<uint8_t> want_boxed((size_t)w * h);
        const DSDTM::BoxResult want = DSDTM::mcd_box_host(m.data(), w, h, stride, want_boxed.data(), w);
        CHECK(want.area2 > 0 && !memcmp(d.box, want.box, sizeof want.box) && d.area2 == want.area2 && d.n_components == want.n_components);
        if (!boxed.empty())
            for (int y = 0; y < h; ++y) for (int x = 0; x < w + 2; ++x) CHECK(boxed[(size_t)y * (w + 2) + x] == (x < w ? want_boxed[(size_t)y * w + x] : 0xA5));
        if (dev) CHECK(!memcmp(dev, m.data(), m.size()));          // the source is not modified
        return true;
    }
    void release() { if (dev) (void)hipFree(dev); dev = nullptr; }
};

static int run_boxes(dsdtm_mcd_ctx* ctx, std::vector<Box>& b) {
    std::vector<dsdtm_mcd_box_desc> d;
    for (auto& x : b) d.push_back(x.d);
    const int rc = dsdtm_mcd_boxes(ctx, (int)d.size(), d.data());
    for (size_t k = 0; k < b.size(); ++k) b[k].d = d[k];
    return rc;
}

static bool boxes_failures() {
    dsdtm_mcd_ctx* ctx = nullptr;
    CHECK(dsdtm_mcd_create(0, &ctx) == DSDTM_OK);
    std::vector<Box> b(4);
    CHECK(b[0].init(64, 48, 64, false, true) && b[1].init(40, 24, 64, true, true) && b[2].init(37, 29, 41, false, false) && b[3].init(131, 67, 140, true, true));
    CHECK(run_boxes(ctx, b) == DSDTM_OK);
    for (auto& x : b) { CHECK(x.answered()); x.prefill(); }
    const size_t live0 = fake_hip_live_allocations();
    const long c0 = fake_hip_calls("hipMemcpyAsync"), y0 = fake_hip_calls("hipStreamSynchronize"), l0 = fake_contour_launches();
    CHECK(run_boxes(ctx, b) == DSDTM_OK);
    for (auto& x : b) { CHECK(x.answered()); x.prefill(); }
    const long copies = fake_hip_calls("hipMemcpyAsync") - c0, waits = fake_hip_calls("hipStreamSynchronize") - y0;
    CHECK(copies == 2 && waits == 3 && fake_contour_launches() == l0 + 1);          // one upload, one read-back; two launches' drains and the wait
    auto failed_cleanly = [&](int rc) {
        CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_mcd_last_error(ctx)) > 0);
        for (auto& x : b) CHECK(x.untouched());
        CHECK(run_boxes(ctx, b) == DSDTM_OK);
        for (auto& x : b) { CHECK(x.answered()); x.prefill(); }
        return true;
    };
    for (long nth = 1; nth <= copies; ++nth) { fake_hip_fail("hipMemcpyAsync", nth); const int rc = run_boxes(ctx, b); fake_hip_fail("hipMemcpyAsync", 0); CHECK(failed_cleanly(rc)); }
    for (long nth = 1; nth <= waits; ++nth) { fake_hip_fail("hipStreamSynchronize", nth); const int rc = run_boxes(ctx, b); fake_hip_fail("hipStreamSynchronize", 0); CHECK(failed_cleanly(rc)); }
    for (long nth = 1; nth <= 2; ++nth) { fake_contour_fail(nth); const int rc = run_boxes(ctx, b); fake_contour_fail(0); CHECK(failed_cleanly(rc)); }
    CHECK(fake_hip_live_allocations() == live0);
    // nobody wants a boxed mask: no fill launch
    const long f0 = fake_contour_fill_launches();
    std::vector<Box> q(1);
    CHECK(q[0].init(37, 29, 41, false, false) && run_boxes(ctx, q) == DSDTM_OK && q[0].answered() && fake_contour_fill_launches() == f0);
    for (auto& x : b) x.release();
    dsdtm_mcd_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// n = 0 and its limits, a duplicate model, sizes the contour step refuses, a desc rejected in the middle, the fields the checks name
static bool argument_checks() {
    dsdtm_mcd_ctx *ctx = nullptr, *other = nullptr;
    CHECK(dsdtm_mcd_create(0, &ctx) == DSDTM_OK && dsdtm_mcd_create(0, &other) == DSDTM_OK);
    const long l0 = fake_motion_step_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    CHECK(dsdtm_mcd_steps(ctx, 0, nullptr) == DSDTM_OK && dsdtm_mcd_boxes(ctx, 0, nullptr) == DSDTM_OK);
    CHECK(fake_motion_step_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);          // nothing done
    CHECK(dsdtm_mcd_steps(ctx, -1, nullptr) == DSDTM_ERR_INVALID && dsdtm_mcd_steps(ctx, 3, nullptr) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_mcd_boxes(ctx, -1, nullptr) == DSDTM_ERR_INVALID && dsdtm_mcd_boxes(ctx, 3, nullptr) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_mcd_steps(nullptr, 0, nullptr) == DSDTM_ERR_INVALID && dsdtm_mcd_boxes(nullptr, 0, nullptr) == DSDTM_ERR_INVALID);
    std::vector<Step> s(3);
    CHECK(s[0].init(ctx, 64, 48, 64, 6, false) && s[1].init(ctx, 70, 50, 70, 0, false) && s[2].init(ctx, 70, 50, 72, 1, true));
    std::vector<dsdtm_mcd_desc> big((size_t)DSDTM_MOTION_STEPS_MAX + 1, s[0].d);
    CHECK(dsdtm_mcd_steps(ctx, DSDTM_MOTION_STEPS_MAX + 1, big.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_mcd_last_error(ctx), "n ="));
    auto invalid = [&](const char* what) {
        const long l1 = fake_motion_step_launches();
        const int rc = run(ctx, s);
        bool ok = rc == DSDTM_ERR_INVALID && strstr(dsdtm_mcd_last_error(ctx), what) && fake_motion_step_launches() == l1 && fake_hip_pending() == 0;
        for (auto& x : s) ok = ok && x.untouched() && x.generation(ctx, 1.0f);
        if (!ok) std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_mcd_last_error(ctx));
        return ok;
    };
    s[2].d.model = s[1].model; CHECK(invalid("model 2") && strstr(dsdtm_mcd_last_error(ctx), "model 1")); s[2].d.model = s[2].model;
    s[1].H[7] = std::numeric_limits<double>::quiet_NaN(); CHECK(invalid("model 1: H")); s[1].H[7] = 0;
    const dsdtm_mcd_desc good = s[0].d;
    s[0].d.image = nullptr; CHECK(invalid("image")); s[0].d = good;
    s[0].d.model = nullptr; CHECK(invalid("model is NULL")); s[0].d = good;
    s[0].d.stride = 63; CHECK(invalid("stride")); s[0].d = good;
    s[0].d.mask_stride = 63; CHECK(invalid("mask_stride")); s[0].d = good;
    s[0].d.mask_raw_stride = 63; CHECK(invalid("mask_raw_stride")); s[0].d = good;
    s[0].d.n_features = DSDTM_MOTION_MAX_FEATURES + 1; CHECK(invalid("n_features")); s[0].d = good;
    s[0].d.feature_on_mask = nullptr; CHECK(invalid("feature_on_mask")); s[0].d = good;
    s[0].feat[2 * 4] = 63.5f; CHECK(invalid("feature 4")); s[0].feat[2 * 4] = 63.49f;   // 63.5 rounds to 64 (even): outside
    CHECK(run(other, s) == DSDTM_ERR_INVALID && strstr(dsdtm_mcd_last_error(other), "another context"));
    // a model larger than the contour step takes: it can be made, read and reset; the step names the size
    dsdtm_mcd_model* huge = nullptr;
    CHECK(dsdtm_mcd_model_create(ctx, 1025, 1024, &huge) == DSDTM_OK && dsdtm_mcd_model_reset(ctx, huge) == DSDTM_OK);
    std::vector<uint8_t> himg((size_t)1025 * 1024, 0);
    s[1].d.model = huge; s[1].d.image = himg.data(); s[1].d.stride = 1025; s[1].d.mask = nullptr; s[1].d.mask_raw = nullptr;
    const dsdtm_mcd_desc keep1 = s[1].d;
    {
        const int rc = run(ctx, s);
        CHECK(rc == DSDTM_ERR_INVALID && strstr(dsdtm_mcd_last_error(ctx), "1025 x 1024") && strstr(dsdtm_mcd_last_error(ctx), "1048576"));
        CHECK(s[0].untouched() && s[0].generation(ctx, 1.0f));
    }
    (void)keep1;
    dsdtm_mcd_model_destroy(ctx, huge);
    s[1].d.model = s[1].model; s[1].d.image = s[1].img.data(); s[1].d.stride = 70; s[1].d.mask = s[1].mask.data(); s[1].d.mask_raw = s[1].raw.data();
    CHECK(run(ctx, s) == DSDTM_OK);
    for (auto& x : s) CHECK(x.answered() && x.generation(ctx, 2.0f));
    // boxes
    std::vector<Box> b(2);
    CHECK(b[0].init(64, 48, 64, false, true) && b[1].init(40, 24, 64, true, true));
    auto box_invalid = [&](const char* what) {
        const long k0 = fake_contour_launches();
        const int rc = run_boxes(ctx, b);
        const bool ok = rc == DSDTM_ERR_INVALID && strstr(dsdtm_mcd_last_error(ctx), what) && fake_contour_launches() == k0 && b[0].untouched() && b[1].untouched();
        if (!ok) std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_mcd_last_error(ctx));
        return ok;
    };
    const dsdtm_mcd_box_desc bgood = b[1].d;
    b[1].d.mask = nullptr; CHECK(box_invalid("mask 1: mask is NULL")); b[1].d = bgood;
    b[1].d.width = 15; CHECK(box_invalid("width")); b[1].d = bgood;
    b[1].d.height = 4097; CHECK(box_invalid("height")); b[1].d = bgood;
    b[1].d.stride = 39; CHECK(box_invalid("stride")); b[1].d = bgood;
    b[1].d.boxed_stride = 39; CHECK(box_invalid("boxed_stride")); b[1].d = bgood;
    b[1].d.mask = himg.data(); b[1].d.width = 1025; b[1].d.height = 1024; b[1].d.stride = 1025; b[1].d.boxed = nullptr;
    CHECK(box_invalid("1025 x 1024")); b[1].d = bgood;
    CHECK(run_boxes(ctx, b) == DSDTM_OK && b[0].answered() && b[1].answered());
    for (auto& x : b) x.release();
    for (auto& x : s) x.release(ctx);
    dsdtm_mcd_destroy(other);
    dsdtm_mcd_destroy(ctx);
    dsdtm_mcd_destroy(nullptr);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_mcd", dsdtm_mcd_create, dsdtm_mcd_destroy, dsdtm_mcd_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"step_failures", step_failures}, {"boxes_failures", boxes_failures},
                                                      {"argument_checks", argument_checks}, {"create_failures", create_failures}};
    int failed = 0;
    for (const auto& sc : all) {
        bool wanted = argc < 2;
        for (int i = 1; i < argc; ++i) wanted = wanted || sc.first == argv[i];
        if (!wanted) continue;
        fake_hip_reset();
        const bool ok = sc.second();
        std::printf("%s %s\n", ok ? "ok" : "FAILED", sc.first.c_str());
        std::fflush(stdout);
        failed += ok ? 0 : 1;
    }
    return failed ? 1 : 0;
}
