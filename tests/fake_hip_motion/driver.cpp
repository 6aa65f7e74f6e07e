// libdsdtm_amd_motion.so's host side (dsdtm_amd/csrc/motion_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified):
// contexts and models, the checks, the packing of n steps into one block, the one upload / one launch / read-back, every failure
// path — as a stand-alone program under ASan/UBSan/LSan. The launches are the fakes of tests/fake_hip_motion/fake_motion.cpp.
// Test infrastructure (tests/test_motion_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_motion.h"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_motion.h"

static const double IDENT[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

// one model's step: image (host, or "device" = hipMalloc of the fake), outputs prefilled with 0xA5
struct Step {
    int w = 0, h = 0, stride = 0, nf = 0;
    dsdtm_motion_model* model = nullptr;
    std::vector<uint8_t> img, mask, flags;
    std::vector<float> feat;
    uint8_t* dev_img = nullptr;
    double H[9];
    dsdtm_motion_desc d{};
    bool init(dsdtm_motion_ctx* ctx, int w_, int h_, int stride_, int nf_, bool device_image, bool want_mask = true) {
        w = w_; h = h_; stride = stride_; nf = nf_;
        memcpy(H, IDENT, sizeof H);
        CHECK(dsdtm_motion_model_create(ctx, w, h, &model) == DSDTM_OK && model);
        img.resize((size_t)stride * h);
        for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)((i * 37 + (size_t)w) % 251);
        if (device_image) {
            CHECK(hipMalloc((void**)&dev_img, img.size()) == hipSuccess);
            memcpy(dev_img, img.data(), img.size());
        }
        mask.resize(want_mask ? (size_t)(w + 3) * h : 0);
        flags.resize((size_t)nf);
        feat.resize(2 * (size_t)nf);
        for (int f = 0; f < nf; ++f) { feat[2 * f] = (float)((f * 7) % w) + 0.25f; feat[2 * f + 1] = (float)((f * 5) % (h - 1)) + 0.5f * (f % 2); }
        d.model = model; d.image = device_image ? dev_img : img.data(); d.stride = stride; d.H = H;
        d.mask = want_mask ? mask.data() : nullptr; d.mask_stride = w + 3;
        d.n_features = nf; d.feature_px = nf ? feat.data() : nullptr; d.feature_on_mask = nf ? flags.data() : nullptr;
        prefill();
        return true;
    }
    void prefill() { fill_a5(mask.data(), mask.size()); fill_a5(flags.data(), flags.size()); }
    bool untouched() const { return all_a5(mask.data(), mask.size()) && all_a5(flags.data(), flags.size()); }
    uint8_t on(int x, int y) const { return img[(size_t)y * stride + x] >= 128 ? 255 : 0; }
    bool answered() const {          // what the fake launches leave (fake_motion.cpp)
        if (!mask.empty())
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w + 3; ++x) CHECK(mask[(size_t)y * (w + 3) + x] == (x < w ? on(x, y) : 0xA5));
        for (int f = 0; f < nf; ++f) CHECK(flags[f] == (on((int)nearbyintf(feat[2 * f]), (int)nearbyintf(feat[2 * f + 1])) == 255 ? 1 : 0));
        return true;
    }
    // the fake writes src + 1 everywhere: the model's generation count
    bool generation(dsdtm_motion_ctx* ctx, float want) const {
        std::vector<float> st(12 * (size_t)(w / 4) * (size_t)(h / 4), -1.0f);
        CHECK(dsdtm_motion_model_read(ctx, model, st.data()) == DSDTM_OK);
        for (float v : st) CHECK(v == want);
        return true;
    }
    void release(dsdtm_motion_ctx* ctx) {
        dsdtm_motion_model_destroy(ctx, model); model = nullptr;
        if (dev_img) (void)hipFree(dev_img);
        dev_img = nullptr;
    }
};

static int run(dsdtm_motion_ctx* ctx, std::vector<Step>& s) {
    std::vector<dsdtm_motion_desc> d;
    for (auto& x : s) d.push_back(x.d);
    return dsdtm_motion_steps(ctx, (int)d.size(), d.data());
}

// every copy, launch and wait of a step / a batch failing once (and the allocations of a staging block that must grow): an error,
// the outputs and the models' generations untouched, nothing pending, nothing leaked; the next call succeeds
static bool step_failures() {
    dsdtm_motion_ctx* ctx = nullptr;
    CHECK(dsdtm_motion_create(0, &ctx) == DSDTM_OK);
    std::vector<Step> s(3);
    CHECK(s[0].init(ctx, 64, 48, 64, 20, false) && s[1].init(ctx, 70, 50, 80, 0, true) && s[2].init(ctx, 33, 17, 40, 5, false, false));
    float gen = 1.0f;                                       // ProbModel::init was one launch
    for (auto& x : s) CHECK(x.generation(ctx, gen));
    CHECK(run(ctx, s) == DSDTM_OK);
    gen += 1.0f;
    for (auto& x : s) { CHECK(x.answered() && x.generation(ctx, gen)); x.prefill(); }
    const size_t live0 = fake_hip_live_allocations();
    auto failed_cleanly = [&](int rc) {
        CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_motion_last_error(ctx)) > 0);
        for (auto& x : s) CHECK(x.untouched() && x.generation(ctx, gen));
        CHECK(run(ctx, s) == DSDTM_OK);
        gen += 1.0f;
        for (auto& x : s) { CHECK(x.answered() && x.generation(ctx, gen)); x.prefill(); }
        return true;
    };
    for (long nth = 1; nth <= 3; ++nth) {                   // the upload, the flags' read-back, the masks' read-back
        fake_hip_fail("hipMemcpyAsync", nth);
        const int rc = run(ctx, s);
        fake_hip_fail("hipMemcpyAsync", 0);
        CHECK(failed_cleanly(rc));
    }
    for (long nth = 1; nth <= 3; ++nth) {                   // the two launches' drains, the wait
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
    // the single entry is the batch entry with n = 1
    fake_hip_fail("hipMemcpyAsync", 1);
    CHECK(dsdtm_motion_step(ctx, s[0].model, s[0].d.image, 64, IDENT, s[0].mask.data(), 67, 20, s[0].feat.data(), s[0].flags.data()) == DSDTM_ERR_HIP);
    fake_hip_fail("hipMemcpyAsync", 0);
    CHECK(s[0].untouched() && s[0].generation(ctx, gen));
    CHECK(dsdtm_motion_step(ctx, s[0].model, s[0].d.image, 64, IDENT, s[0].mask.data(), 67, 20, s[0].feat.data(), s[0].flags.data()) == DSDTM_OK);
    CHECK(s[0].answered() && s[0].generation(ctx, gen + 1.0f) && s[1].generation(ctx, gen));
    CHECK(fake_hip_live_allocations() == live0);
    // a fresh context whose staging block cannot be had: pinned, then device
    for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
        dsdtm_motion_ctx* c2 = nullptr;
        CHECK(dsdtm_motion_create(0, &c2) == DSDTM_OK);
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
        dsdtm_motion_destroy(c2);
    }
    for (auto& x : s) x.release(ctx);
    dsdtm_motion_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// model_create, reset, read and write: every allocation, copy, launch and wait failing once
static bool model_failures() {
    dsdtm_motion_ctx* ctx = nullptr;
    CHECK(dsdtm_motion_create(0, &ctx) == DSDTM_OK);
    const size_t live0 = fake_hip_live_allocations();
    dsdtm_motion_model* m = (dsdtm_motion_model*)(uintptr_t)1;
    struct Point { const char* api; long nth; };
    const Point create_points[] = {{"hipMalloc", 1}, {"hipHostMalloc", 1}, {"hipMalloc", 2}, {"hipMemcpyAsync", 1}, {"hipStreamSynchronize", 1}, {"hipStreamSynchronize", 2}};
    for (const Point& p : create_points) {
        fake_hip_fail(p.api, p.nth);
        const int rc = dsdtm_motion_model_create(ctx, 64, 48, &m);
        fake_hip_fail(p.api, 0);
        CHECK(rc == DSDTM_ERR_HIP && m == nullptr && fake_hip_pending() == 0 && strlen(dsdtm_motion_last_error(ctx)) > 0);
        m = (dsdtm_motion_model*)(uintptr_t)1;
    }
    fake_motion_fail(1);
    CHECK(dsdtm_motion_model_create(ctx, 64, 48, &m) == DSDTM_ERR_HIP && m == nullptr);
    fake_motion_fail(0);
    CHECK(dsdtm_motion_model_create(ctx, 64, 48, &m) == DSDTM_OK && m);
    const size_t cells = 16 * 12;
    std::vector<float> st(12 * cells, -7.0f), in(12 * cells);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (float)i * 0.5f;
    // read: the copy, the wait
    for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize"}) {
        fake_hip_fail(api, 1);
        CHECK(dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_ERR_HIP && fake_hip_pending() == 0);
        fake_hip_fail(api, 0);
        for (float v : st) CHECK(v == -7.0f);
    }
    CHECK(dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK);
    for (float v : st) CHECK(v == 1.0f);
    // write: a failure leaves the model as it was
    for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize"}) {
        fake_hip_fail(api, 1);
        CHECK(dsdtm_motion_model_write(ctx, m, in.data()) == DSDTM_ERR_HIP && fake_hip_pending() == 0);
        fake_hip_fail(api, 0);
        CHECK(dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK);
        for (float v : st) CHECK(v == 1.0f);
    }
    CHECK(dsdtm_motion_model_write(ctx, m, in.data()) == DSDTM_OK && dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK && st == in);
    // reset: a failure leaves the model as it was; a success is ProbModel::init again
    for (const Point& p : {Point{"hipMemcpyAsync", 1}, Point{"hipStreamSynchronize", 1}, Point{"hipStreamSynchronize", 2}}) {
        fake_hip_fail(p.api, p.nth);
        CHECK(dsdtm_motion_model_reset(ctx, m) == DSDTM_ERR_HIP && fake_hip_pending() == 0);
        fake_hip_fail(p.api, 0);
        CHECK(dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK && st == in);
    }
    fake_motion_fail(1);
    CHECK(dsdtm_motion_model_reset(ctx, m) == DSDTM_ERR_HIP);
    fake_motion_fail(0);
    CHECK(dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK && st == in);
    CHECK(dsdtm_motion_model_reset(ctx, m) == DSDTM_OK && dsdtm_motion_model_read(ctx, m, st.data()) == DSDTM_OK);
    for (float v : st) CHECK(v == 1.0f);
    CHECK(dsdtm_motion_model_read(ctx, m, nullptr) == DSDTM_ERR_INVALID && dsdtm_motion_model_write(ctx, m, nullptr) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_motion_model_read(ctx, nullptr, st.data()) == DSDTM_ERR_INVALID && dsdtm_motion_model_reset(ctx, nullptr) == DSDTM_ERR_INVALID);
    dsdtm_motion_model_destroy(ctx, m);
    dsdtm_motion_model_destroy(ctx, nullptr);
    dsdtm_motion_destroy(ctx);
    CHECK(fake_hip_live_allocations() <= live0);
    CHECK(fake_hip_errors().empty());
    return true;
}

// n = 0; n at and over its limit; ONE launch for a batch; a duplicate model; a desc rejected in the middle
static bool batch_rules() {
    dsdtm_motion_ctx* ctx = nullptr;
    CHECK(dsdtm_motion_create(0, &ctx) == DSDTM_OK);
    const long l0 = fake_motion_step_launches(), f0 = fake_motion_feature_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    CHECK(dsdtm_motion_steps(ctx, 0, nullptr) == DSDTM_OK);
    CHECK(fake_motion_step_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);          // nothing done
    CHECK(dsdtm_motion_steps(ctx, -1, nullptr) == DSDTM_ERR_INVALID && dsdtm_motion_steps(ctx, 3, nullptr) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_motion_steps(nullptr, 0, nullptr) == DSDTM_ERR_INVALID);
    std::vector<Step> s(5);
    CHECK(s[0].init(ctx, 64, 48, 64, 3, false) && s[1].init(ctx, 70, 50, 70, 0, false) && s[2].init(ctx, 16, 16, 16, 1, true) &&
          s[3].init(ctx, 128, 20, 130, 40, true, false) && s[4].init(ctx, 70, 50, 72, 0, false, false));
    const long l1 = fake_motion_step_launches();
    CHECK(run(ctx, s) == DSDTM_OK && fake_motion_step_launches() == l1 + 1 && fake_motion_feature_launches() == f0 + 1);
    for (auto& x : s) { CHECK(x.answered() && x.generation(ctx, 2.0f)); x.prefill(); }
    std::vector<dsdtm_motion_desc> big((size_t)DSDTM_MOTION_STEPS_MAX + 1, s[0].d);
    CHECK(dsdtm_motion_steps(ctx, DSDTM_MOTION_STEPS_MAX + 1, big.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_motion_last_error(ctx), "n ="));
    // the same model twice: refused, named, nothing enqueued, every model as it was
    const long l2 = fake_motion_step_launches(), c2 = fake_hip_calls("hipMemcpyAsync");
    s[4].d.model = s[1].model;
    CHECK(run(ctx, s) == DSDTM_ERR_INVALID && strstr(dsdtm_motion_last_error(ctx), "model 4") && strstr(dsdtm_motion_last_error(ctx), "model 1"));
    s[4].d.model = s[4].model;
    CHECK(fake_motion_step_launches() == l2 && fake_hip_calls("hipMemcpyAsync") == c2 && fake_hip_pending() == 0);
    for (auto& x : s) CHECK(x.untouched() && x.generation(ctx, 2.0f));
    // a desc rejected in the middle: all or nothing
    s[2].H[7] = std::numeric_limits<double>::quiet_NaN();
    CHECK(run(ctx, s) == DSDTM_ERR_INVALID && strstr(dsdtm_motion_last_error(ctx), "model 2: H"));
    s[2].H[7] = 0;
    for (auto& x : s) CHECK(x.untouched() && x.generation(ctx, 2.0f));
    CHECK(fake_motion_step_launches() == l2);
    CHECK(run(ctx, s) == DSDTM_OK);
    for (auto& x : s) CHECK(x.answered() && x.generation(ctx, 3.0f));
    for (auto& x : s) x.release(ctx);
    dsdtm_motion_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool argument_checks() {
    dsdtm_motion_ctx *ctx = nullptr, *other = nullptr;
    CHECK(dsdtm_motion_create(0, &ctx) == DSDTM_OK && dsdtm_motion_create(0, &other) == DSDTM_OK);
    dsdtm_motion_model* m = nullptr;
    for (int bad : {15, 0, -4, 4097}) {
        CHECK(dsdtm_motion_model_create(ctx, bad, 48, &m) == DSDTM_ERR_INVALID && !m && strstr(dsdtm_motion_last_error(ctx), "width"));
        CHECK(dsdtm_motion_model_create(ctx, 64, bad, &m) == DSDTM_ERR_INVALID && !m && strstr(dsdtm_motion_last_error(ctx), "height"));
    }
    CHECK(dsdtm_motion_model_create(ctx, 64, 48, nullptr) == DSDTM_ERR_INVALID);
    std::vector<Step> s(1);
    CHECK(s[0].init(ctx, 64, 48, 64, 6, false));
    const long l0 = fake_motion_step_launches();
    auto invalid = [&](const char* what) {
        const int rc = run(ctx, s);
        if (rc != DSDTM_ERR_INVALID || !s[0].untouched() || !strstr(dsdtm_motion_last_error(ctx), what)) {
            std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_motion_last_error(ctx));
            return false;
        }
        return true;
    };
    const dsdtm_motion_desc good = s[0].d;
    s[0].d.image = nullptr; CHECK(invalid("image")); s[0].d = good;
    s[0].d.model = nullptr; CHECK(invalid("model is NULL")); s[0].d = good;
    s[0].d.H = nullptr; CHECK(invalid("H is NULL")); s[0].d = good;
    s[0].d.stride = 63; CHECK(invalid("stride")); s[0].d = good;
    s[0].d.mask_stride = 63; CHECK(invalid("mask_stride")); s[0].d = good;
    s[0].d.n_features = -1; CHECK(invalid("n_features")); s[0].d = good;
    s[0].d.n_features = DSDTM_MOTION_MAX_FEATURES + 1; CHECK(invalid("n_features")); s[0].d = good;
    s[0].d.feature_px = nullptr; CHECK(invalid("feature_px")); s[0].d = good;
    s[0].d.feature_on_mask = nullptr; CHECK(invalid("feature_on_mask")); s[0].d = good;
    s[0].H[2] = std::numeric_limits<double>::infinity(); CHECK(invalid("H is not finite")); s[0].H[2] = 0;
    s[0].H[8] = 0.0; CHECK(invalid("denominator")); s[0].H[8] = 1.0;                    // 0 at every cell
    s[0].H[6] = -1.0 / 61.0; CHECK(invalid("denominator")); s[0].H[6] = 0.0;            // positive at the left corners only (X = 62 at the right)
    s[0].H[7] = -1.0 / 45.0; CHECK(invalid("denominator")); s[0].H[7] = 0.0;            // (Y = 46 at the bottom)
    s[0].H[6] = -1.0 / 63.0; CHECK(run(ctx, s) == DSDTM_OK && s[0].answered()); s[0].H[6] = 0.0; s[0].prefill();      // still positive at X = 62
    s[0].feat[2 * 4] = 63.5f; CHECK(invalid("feature 4")); s[0].feat[2 * 4] = 63.49f;   // 63.5 rounds to 64 (even): outside
    s[0].feat[2 * 5 + 1] = -0.51f; CHECK(invalid("feature 5")); s[0].feat[2 * 5 + 1] = -0.5f;      // -0.5 rounds to -0: inside
    s[0].feat[0] = std::numeric_limits<float>::quiet_NaN(); CHECK(invalid("feature 0")); s[0].feat[0] = 0.0f;
    CHECK(fake_motion_step_launches() == l0 + 1);
    CHECK(run(other, s) == DSDTM_ERR_INVALID && strstr(dsdtm_motion_last_error(other), "another context") && s[0].untouched());
    CHECK(run(ctx, s) == DSDTM_OK && s[0].answered());
    // an image in "device" memory with an offset into its allocation and a stride: read where it is
    std::vector<Step> one(1);
    CHECK(one[0].init(ctx, 32, 24, 50, 4, true));
    one[0].d.image = one[0].dev_img + 7;            // (the last row then ends 7 bytes short of the allocation's end: 23 * 50 + 7 + 32 <= 24 * 50)
    for (size_t i = 0; i + 7 < one[0].img.size(); ++i) one[0].img[i] = one[0].dev_img[i + 7];
    CHECK(run(ctx, one) == DSDTM_OK && one[0].answered());
    one[0].release(ctx);
    s[0].release(ctx);
    dsdtm_motion_destroy(other);
    dsdtm_motion_destroy(ctx);
    dsdtm_motion_destroy(nullptr);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_motion", dsdtm_motion_create, dsdtm_motion_destroy, dsdtm_motion_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"step_failures", step_failures}, {"model_failures", model_failures},
                                                      {"batch_rules", batch_rules}, {"argument_checks", argument_checks},
                                                      {"create_failures", create_failures}};
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
