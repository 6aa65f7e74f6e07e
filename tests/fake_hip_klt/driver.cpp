// libdsdtm_amd_klt.so's host side (dsdtm_amd/csrc/klt_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified): models, the
// first step, the pyramid swap, reset, the three memory kinds of an image, the read-back split between models that asked for their
// correspondences and those that did not, every refusal and every HIP call failing in turn, destroy behind a failed step — as a
// stand-alone program under ASan/UBSan/LSan. The launches are the fakes of fake_klt.cpp, tests/fake_hip_homography/fake_homography.cpp and the runtime's own pyrdown_launch.
// Test infrastructure (tests/test_klt_cpu.py); nothing here is part of the product.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_klt.h"
#include "../../dsdtm_amd/host/dsdtm_klt_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_homography.h"
#include "fake_klt.h"

enum Mem { PAGEABLE, PINNED, DEVICE };

// the pyramid as the fake runtime builds it: level 0 is the image, its pyrdown_launch fills every other level with 0x11
static std::vector<DSDTM::KltLevel> fake_pyramid(const uint8_t* image, int w, int h, int stride, int levels, std::vector<std::vector<uint8_t>>& store) {
    std::vector<DSDTM::KltLevel> p = DSDTM::klt_pyramid_host(image, w, h, stride, levels, store);
    for (auto& l : store) std::fill(l.begin(), l.end(), (uint8_t)0x11);
    return p;
}

struct Buf {
    void* p = nullptr; size_t bytes = 0; Mem mem = PAGEABLE;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    void release() {
        if (!p) return;
        if (mem == PAGEABLE) free(p); else if (mem == PINNED) (void)hipHostFree(p); else (void)hipFree(p);
        p = nullptr;
    }
    bool make(Mem m, size_t n) {
        release();
        mem = m; bytes = n;
        if (m == PAGEABLE) { p = malloc(n); return p != nullptr; }
        return (m == PINNED ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n)) == hipSuccess;
    }
};

// a smooth pattern whose content lies `shift` pixels further right; the buffer holds exactly (h - 1) stride + w bytes
static bool image(Buf& b, Mem mem, int w, int h, int stride, int shift) {
    CHECK(b.make(mem, (size_t)(h - 1) * stride + w));
    memset(b.p, 0x11, b.bytes);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            ((uint8_t*)b.p)[(size_t)y * stride + x] = (uint8_t)(128.0 + 60.0 * std::sin((x - shift) * 0.35) + 50.0 * std::cos(y * 0.3 + (x - shift) * 0.1));
    return true;
}

// one tracker: a model, two images, the optional output arrays prefilled with 0xA5
struct Tracker {
    int w = 0, h = 0, levels = 0, gw = 0, gh = 0, stride = 0, np = 0;
    bool want = false;
    dsdtm_klt_model* model = nullptr;
    Buf img[2];
    std::vector<float> prev_points, points;
    std::vector<uint8_t> status, mask;
    std::vector<int32_t> iterations;
    bool init(dsdtm_klt_ctx* ctx, int w_, int h_, int levels_, int gw_, int gh_, Mem mem, int pad, bool want_) {
        w = w_; h = h_; levels = levels_; gw = gw_; gh = gh_; stride = w + pad; want = want_;
        np = (int)DSDTM::klt_grid_host(w, h, gw, gh).size() / 2;
        CHECK(dsdtm_klt_model_create(ctx, w, h, levels, &model) == DSDTM_OK && model);
        CHECK(image(img[0], mem, w, h, stride, 0) && image(img[1], mem, w, h, stride, 1));
        prev_points.assign((size_t)np * 2, 0); points.assign((size_t)np * 2, 0); status.assign((size_t)np, 0); mask.assign((size_t)np, 0); iterations.assign((size_t)np, 0);
        prefill();
        return true;
    }
    void prefill() {
        fill_a5(prev_points.data(), prev_points.size() * 4); fill_a5(points.data(), points.size() * 4); fill_a5(status.data(), status.size());
        fill_a5(mask.data(), mask.size()); fill_a5(iterations.data(), iterations.size() * 4);
    }
    bool untouched() const {
        return all_a5(prev_points.data(), prev_points.size() * 4) && all_a5(points.data(), points.size() * 4) && all_a5(status.data(), status.size()) &&
               all_a5(mask.data(), mask.size()) && all_a5(iterations.data(), iterations.size() * 4);
    }
    dsdtm_klt_desc desc(int which) {
        dsdtm_klt_desc d{};
        d.model = model; d.image = (const uint8_t*)img[which].p; d.stride = stride; d.grid_w = gw; d.grid_h = gh;
        if (want) { d.prev_points = prev_points.data(); d.points = points.data(); d.status = status.data(); d.iterations = iterations.data(); d.mask = mask.data(); }
        return d;
    }
    // what a step from image `from` to image `to` must answer (from < 0: a first step), by the host functions and the fakes' rules
    bool answered(const dsdtm_klt_result& r, int from, int to, int frame) const {
        CHECK(r.n_points == np && r.frame == frame);
        const std::vector<float> grid = DSDTM::klt_grid_host(w, h, gw, gh);
        if (want) CHECK(memcmp(prev_points.data(), grid.data(), grid.size() * 4) == 0);
        if (from < 0) {
            CHECK(r.source == DSDTM_KLT_SOURCE_IDENTITY && r.n_tracked == 0 && r.H[0] == 1.0 && r.H[4] == 1.0 && r.H[8] == 1.0 && r.H[2] == 0.0);
            if (want) {
                CHECK(memcmp(points.data(), grid.data(), grid.size() * 4) == 0 && all_a5(mask.data(), mask.size()));
                for (int k = 0; k < np; ++k) CHECK(status[(size_t)k] == 0 && iterations[(size_t)k] == 0);
            }
            return true;
        }
        std::vector<uint8_t> a((size_t)w * h), b((size_t)w * h);          // (device images are plain memory to the fake)
        for (int y = 0; y < h; ++y) {
            memcpy(a.data() + (size_t)y * w, (const uint8_t*)img[from].p + (size_t)y * stride, (size_t)w);
            memcpy(b.data() + (size_t)y * w, (const uint8_t*)img[to].p + (size_t)y * stride, (size_t)w);
        }
        std::vector<std::vector<uint8_t>> s0, s1;
        const std::vector<DSDTM::KltLevel> p0 = fake_pyramid(a.data(), w, h, w, levels, s0), p1 = fake_pyramid(b.data(), w, h, w, levels, s1);
        const DSDTM::KltStepHost hs = DSDTM::klt_step_host(p0.data(), p1.data(), levels, gw, gh);
        CHECK(hs.n_points == np && r.n_tracked == hs.n_tracked);
        if (want) {
            CHECK(memcmp(points.data(), hs.points.data(), hs.points.size() * 4) == 0 && memcmp(status.data(), hs.status.data(), hs.status.size()) == 0 &&
                  memcmp(iterations.data(), hs.iterations.data(), hs.iterations.size() * 4) == 0);
        }
        if (hs.n_tracked < DSDTM_KLT_MIN_TRACKED) {
            CHECK(r.source == DSDTM_KLT_SOURCE_IDENTITY && r.H[0] == 1.0 && r.H[1] == 0.0 && r.n_inliers == 0);
            if (want) CHECK(all_a5(mask.data(), mask.size()));
            return true;
        }
        double sum = 0;                                   // the fake homography: H[j] = the sum of A's coordinates + j, every point an inlier
        for (float v : hs.a) sum += (double)v;
        CHECK(r.source == DSDTM_KLT_SOURCE_RANSAC && r.n_inliers == hs.n_tracked && r.cost_before == 1.0);
        for (int j = 0; j < 9; ++j) CHECK(r.H[j] == sum + j);
        if (want) {
            for (int i = 0; i < hs.n_tracked; ++i) CHECK(mask[(size_t)i] == (hs.a[2 * (size_t)i] >= hs.b[2 * (size_t)i] ? 1 : 0));
            CHECK(all_a5(mask.data() + hs.n_tracked, mask.size() - (size_t)hs.n_tracked));
        }
        return true;
    }
};

struct World {
    dsdtm_klt_ctx* ctx = nullptr;
    Tracker t[4];
    std::vector<dsdtm_klt_result> res;
    bool init() {
        CHECK(dsdtm_klt_create(0, &ctx) == DSDTM_OK);
        // pageable with an odd stride, asked; pinned, not asked; device, asked; a grid of one point (fewer than 10 survivors), asked
        CHECK(t[0].init(ctx, 96, 72, 3, 16, 12, PAGEABLE, 3, true) && t[1].init(ctx, 96, 72, 3, 16, 12, PINNED, 0, false) &&
              t[2].init(ctx, 83, 61, 2, 12, 10, DEVICE, 5, true) && t[3].init(ctx, 70, 60, 2, 0, 0, PAGEABLE, 1, true));
        prefill();
        return true;
    }
    void prefill() { for (auto& x : t) x.prefill(); res.assign(4, dsdtm_klt_result{}); fill_a5(res.data(), res.size() * sizeof(dsdtm_klt_result)); }
    bool untouched() const { for (auto& x : t) if (!x.untouched()) return false; return all_a5(res.data(), res.size() * sizeof(dsdtm_klt_result)); }
    int run(int which) {
        std::vector<dsdtm_klt_desc> d;
        for (auto& x : t) d.push_back(x.desc(which));
        const int rc = dsdtm_klt_steps(ctx, 4, d.data(), res.data());
        if (rc != DSDTM_OK) std::fprintf(stderr, "steps: %d %s\n", rc, dsdtm_klt_last_error(ctx));
        return rc;
    }
    ~World() { for (auto& x : t) { dsdtm_klt_model_destroy(ctx, x.model); x.img[0].release(); x.img[1].release(); } dsdtm_klt_destroy(ctx); }
};

// first steps, second steps (the pyramids swapped), a step back, reset; the batch against the single entry; the pyramid read-back; flow
static bool answers_and_memory_kinds() {
    {
        World s;
        CHECK(s.init());
        s.prefill();
        CHECK(s.run(0) == DSDTM_OK);
        for (int k = 0; k < 4; ++k) CHECK(s.t[k].answered(s.res[(size_t)k], -1, 0, 0));
        s.prefill();
        CHECK(s.run(1) == DSDTM_OK);
        for (int k = 0; k < 4; ++k) CHECK(s.t[k].answered(s.res[(size_t)k], 0, 1, 1));
        CHECK(s.res[0].source == DSDTM_KLT_SOURCE_RANSAC && s.res[3].source == DSDTM_KLT_SOURCE_IDENTITY && s.res[3].n_points == 1);
        s.prefill();
        CHECK(s.run(0) == DSDTM_OK);                    // the swap: now tracked from image 1
        for (int k = 0; k < 4; ++k) CHECK(s.t[k].answered(s.res[(size_t)k], 1, 0, 2));
        // the single entry equals its place in the batch
        // (the single entry has the default grid: tracker 3's; its arrays are not asked for, so they stay as the batch left them)
        const dsdtm_klt_result batch = s.res[3];
        CHECK(dsdtm_klt_model_reset(s.ctx, s.t[3].model) == DSDTM_OK);
        dsdtm_klt_result one;
        s.t[3].want = false;
        CHECK(dsdtm_klt_step(s.ctx, s.t[3].model, (const uint8_t*)s.t[3].img[1].p, s.t[3].stride, &one) == DSDTM_OK && s.t[3].answered(one, -1, 1, 0));
        CHECK(dsdtm_klt_step(s.ctx, s.t[3].model, (const uint8_t*)s.t[3].img[0].p, s.t[3].stride, &one) == DSDTM_OK && s.t[3].answered(one, 1, 0, 1));
        CHECK(memcmp(one.H, batch.H, sizeof one.H) == 0 && one.n_tracked == batch.n_tracked);
        // the pyramid of the last image, level by level, into a buffer of exactly its size
        Tracker& m = s.t[2];
        std::vector<uint8_t> flat((size_t)m.w * m.h);
        for (int y = 0; y < m.h; ++y) memcpy(flat.data() + (size_t)y * m.w, (const uint8_t*)m.img[0].p + (size_t)y * m.stride, (size_t)m.w);
        std::vector<std::vector<uint8_t>> st;
        const std::vector<DSDTM::KltLevel> p = fake_pyramid(flat.data(), m.w, m.h, m.w, m.levels, st);
        for (int l = 0; l < m.levels; ++l) {
            std::vector<uint8_t> got((size_t)p[(size_t)l].width * p[(size_t)l].height, 0xA5);
            CHECK(dsdtm_klt_model_pyramid(s.ctx, m.model, l, got.data(), p[(size_t)l].width) == DSDTM_OK);
            for (int y = 0; y < p[(size_t)l].height; ++y)
                CHECK(memcmp(got.data() + (size_t)y * p[(size_t)l].width, p[(size_t)l].data + (size_t)y * p[(size_t)l].stride, (size_t)p[(size_t)l].width) == 0);
        }
        // flow: two pairs, one with guesses and all outputs, one with the required output only
        const int n = 5;
        const float pts[2 * n] = {40, 30, 20.5f, 20.25f, 3, 3, 60, 40, 80, 60};
        float guess[2 * n];
        for (int i = 0; i < 2 * n; ++i) guess[i] = pts[i] + 0.5f;
        std::vector<float> out(2 * n), out2(2 * n), res(n), want(2 * n), want_res(n);
        std::vector<uint8_t> stt(n), want_st(n);
        std::vector<int32_t> it(n), want_it(n);
        dsdtm_klt_flow_desc d[2] = {};
        Tracker& a = s.t[0];
        Tracker& b = s.t[2];
        d[0].prev = (const uint8_t*)a.img[0].p; d[0].cur = (const uint8_t*)a.img[1].p; d[0].width = a.w; d[0].height = a.h; d[0].prev_stride = d[0].cur_stride = a.stride;
        d[0].n_points = n; d[0].levels = 2; d[0].window = 7; d[0].points = pts; d[0].guesses = guess; d[0].out_points = out.data(); d[0].status = stt.data();
        d[0].iterations_used = it.data(); d[0].residual = res.data();
        d[1].prev = (const uint8_t*)b.img[1].p; d[1].cur = (const uint8_t*)b.img[0].p; d[1].width = b.w; d[1].height = b.h; d[1].prev_stride = d[1].cur_stride = b.stride;
        d[1].n_points = n; d[1].levels = 1; d[1].points = pts; d[1].out_points = out2.data();
        CHECK(dsdtm_klt_flow(s.ctx, 2, d) == DSDTM_OK);
        {
            std::vector<uint8_t> f0((size_t)a.w * a.h), f1((size_t)a.w * a.h);
            for (int y = 0; y < a.h; ++y) { memcpy(f0.data() + (size_t)y * a.w, (const uint8_t*)a.img[0].p + (size_t)y * a.stride, (size_t)a.w); memcpy(f1.data() + (size_t)y * a.w, (const uint8_t*)a.img[1].p + (size_t)y * a.stride, (size_t)a.w); }
            std::vector<std::vector<uint8_t>> s0, s1;
            const auto p0 = fake_pyramid(f0.data(), a.w, a.h, a.w, 2, s0), p1 = fake_pyramid(f1.data(), a.w, a.h, a.w, 2, s1);
            DSDTM::KltParams P;
            P.window = 7;
            DSDTM::klt_flow_host(p0.data(), p1.data(), 2, n, pts, guess, P, want.data(), want_st.data(), want_it.data(), want_res.data());
            CHECK(memcmp(out.data(), want.data(), out.size() * 4) == 0 && stt == want_st && it == want_it && memcmp(res.data(), want_res.data(), res.size() * 4) == 0);
            CHECK(want_st[0] == 1 && want_st[2] == 0);
        }
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every refusal leaves every output untouched and every model where it was
static bool refusals() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run(0) == DSDTM_OK);
        auto refused = [&](std::vector<dsdtm_klt_desc> d, int n, const char* needle, bool null_results = false) {
            s.prefill();
            const long launches = fake_klt_launches();
            const int rc = dsdtm_klt_steps(s.ctx, n, d.empty() ? nullptr : d.data(), null_results ? nullptr : s.res.data());
            CHECK(rc == DSDTM_ERR_INVALID && s.untouched() && fake_klt_launches() == launches && fake_hip_pending() == 0);
            CHECK(strstr(dsdtm_klt_last_error(s.ctx), needle));
            return true;
        };
        auto descs = [&]() { std::vector<dsdtm_klt_desc> d; for (auto& x : s.t) d.push_back(x.desc(1)); return d; };
        std::vector<dsdtm_klt_desc> d = descs();
        CHECK(refused(d, -1, "outside") && refused(d, DSDTM_KLT_MAX_STEPS + 1, "outside") && refused({}, 4, "descs is NULL") && refused(d, 4, "results is NULL", true));
        d = descs(); d[2].model = nullptr; CHECK(refused(d, 4, "step 2: model is NULL"));
        d = descs(); d[1].image = nullptr; CHECK(refused(d, 4, "step 1: image is NULL"));
        d = descs(); d[3].stride = s.t[3].w - 1; CHECK(refused(d, 4, "step 3: stride"));
        d = descs(); d[0].grid_w = -1; CHECK(refused(d, 4, "step 0: grid_w"));
        d = descs(); d[0].grid_w = 1; d[0].grid_h = 1; CHECK(refused(d, 4, "more than 2048"));
        d = descs(); d[1].model = d[0].model; CHECK(refused(d, 4, "step 1: model appears twice"));      // a model used twice in a call
        CHECK(dsdtm_klt_steps(nullptr, 4, d.data(), s.res.data()) == DSDTM_ERR_INVALID);
        // the models: sizes, levels, NULLs
        dsdtm_klt_model* m = (dsdtm_klt_model*)(uintptr_t)1;
        CHECK(dsdtm_klt_model_create(s.ctx, 40, 120, 4, &m) == DSDTM_ERR_INVALID && m == (dsdtm_klt_model*)(uintptr_t)1 && strstr(dsdtm_klt_last_error(s.ctx), "width"));
        CHECK(dsdtm_klt_model_create(s.ctx, 160, 90, 4, &m) == DSDTM_ERR_INVALID && strstr(dsdtm_klt_last_error(s.ctx), "height"));
        CHECK(dsdtm_klt_model_create(s.ctx, 160, 120, 6, &m) == DSDTM_ERR_INVALID && strstr(dsdtm_klt_last_error(s.ctx), "levels"));
        CHECK(dsdtm_klt_model_create(s.ctx, 160, 120, 4, nullptr) == DSDTM_ERR_INVALID && dsdtm_klt_model_reset(s.ctx, nullptr) == DSDTM_ERR_INVALID);
        uint8_t byte = 0xA5;
        CHECK(dsdtm_klt_model_pyramid(s.ctx, s.t[0].model, 3, &byte, 200) == DSDTM_ERR_INVALID && dsdtm_klt_model_pyramid(s.ctx, s.t[0].model, 0, &byte, 5) == DSDTM_ERR_INVALID && byte == 0xA5);
        dsdtm_klt_model_destroy(s.ctx, nullptr);
        // flow
        const float pts[4] = {40, 30, 20, 20};
        float bad_pts[4] = {40, 30, std::numeric_limits<float>::quiet_NaN(), 20};
        float out[4];
        auto flow_refused = [&](dsdtm_klt_flow_desc f, const char* needle) {
            fill_a5(out, sizeof out);
            CHECK(dsdtm_klt_flow(s.ctx, 1, &f) == DSDTM_ERR_INVALID && all_a5(out, sizeof out) && fake_hip_pending() == 0 && strstr(dsdtm_klt_last_error(s.ctx), needle));
            return true;
        };
        dsdtm_klt_flow_desc f{};
        f.prev = (const uint8_t*)s.t[0].img[0].p; f.cur = (const uint8_t*)s.t[0].img[1].p; f.width = 96; f.height = 72; f.prev_stride = f.cur_stride = s.t[0].stride;
        f.n_points = 2; f.levels = 2; f.points = pts; f.out_points = out;
        dsdtm_klt_flow_desc g = f;
        g.window = 2; CHECK(flow_refused(g, "window")); g = f; g.window = 22; CHECK(flow_refused(g, "window"));
        g = f; g.levels = 6; CHECK(flow_refused(g, "levels")); g = f; g.levels = 4; CHECK(flow_refused(g, "coarsest"));
        g = f; g.prev = nullptr; CHECK(flow_refused(g, "prev is NULL")); g = f; g.out_points = nullptr; CHECK(flow_refused(g, "out_points"));
        g = f; g.n_points = DSDTM_KLT_MAX_FLOW_POINTS + 1; CHECK(flow_refused(g, "n_points")); g = f; g.cur_stride = 95; CHECK(flow_refused(g, "cur_stride"));
        g = f; g.points = bad_pts; CHECK(flow_refused(g, "index 1")); g = f; g.guesses = bad_pts; CHECK(flow_refused(g, "guesses"));
        g = f; g.iterations = 101; CHECK(flow_refused(g, "iterations")); g = f; g.epsilon = -1.0; CHECK(flow_refused(g, "epsilon"));
        // nothing of this moved a model: the next step is every model's second
        s.prefill();
        CHECK(s.run(1) == DSDTM_OK);
        for (int k = 0; k < 4; ++k) CHECK(s.t[k].answered(s.res[(size_t)k], 0, 1, 1));
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

struct Inject { const char* api; long nth; };

// every HIP call and every launch of a step failing in turn: outputs untouched, nothing pending, the models where they were (the
// next step answers as if the failed one had never been called); a model destroyed right behind a failed step, its launches
// enqueued, frees cleanly
static bool call_failures() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run(0) == DSDTM_OK);
        // launches of one call: ingest, (levels - 1) pyrDown per model = 2 + 2 + 1 + 1 (the runtime's own fake), Lucas-Kanade, compaction,
        // the homography's; the three fakes here and the homography's wait once each, the call itself is the fifth wait
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipMemcpyAsync", 1}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 5}, Inject{nullptr, 1},
                          Inject{"pyrdown_launch", 1}, Inject{"pyrdown_launch", 6}, Inject{nullptr, 2}, Inject{nullptr, 3}, Inject{"homography", 1}}) {
            s.prefill();
            if (!in.api) fake_klt_fail(in.nth); else if (!strcmp(in.api, "homography")) fake_homography_fail(1); else fake_hip_fail(in.api, in.nth);
            const int rc = s.run(1);
            if (!in.api) fake_klt_fail(0); else if (!strcmp(in.api, "homography")) fake_homography_fail(0); else fake_hip_fail(in.api, 0);
            CHECK(rc == DSDTM_ERR_HIP && s.untouched() && fake_hip_pending() == 0 && strlen(dsdtm_klt_last_error(s.ctx)) > 0);
        }
        // the staging blocks cannot grow: a fresh context, nothing enqueued
        for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
            dsdtm_klt_ctx* keep = s.ctx;
            CHECK(dsdtm_klt_create(0, &s.ctx) == DSDTM_OK);
            s.prefill();
            fake_hip_fail(api, 1);
            const int rc = s.run(1);
            fake_hip_fail(api, 0);
            CHECK(rc == DSDTM_ERR_HIP && s.untouched() && fake_hip_pending() == 0);
            dsdtm_klt_destroy(s.ctx);
            s.ctx = keep;
        }
        s.prefill();
        CHECK(s.run(1) == DSDTM_OK);
        for (int k = 0; k < 4; ++k) CHECK(s.t[k].answered(s.res[(size_t)k], 0, 1, 1));
        // destroy with a step's buffers in flight: the read-back fails behind the launches, the model goes at once
        const size_t live = fake_hip_live_allocations();
        fake_hip_fail("hipMemcpyAsync", 2);
        CHECK(s.run(0) == DSDTM_ERR_HIP);
        fake_hip_fail("hipMemcpyAsync", 0);
        dsdtm_klt_model_destroy(s.ctx, s.t[0].model);
        s.t[0].model = nullptr;
        CHECK(fake_hip_live_allocations() == live - 1 && fake_hip_pending() == 0);
        // model_create and the pyramid read-back
        dsdtm_klt_model* m = (dsdtm_klt_model*)(uintptr_t)1;
        fake_hip_fail("hipMalloc", 1);
        CHECK(dsdtm_klt_model_create(s.ctx, 96, 72, 3, &m) == DSDTM_ERR_NOMEM && m == (dsdtm_klt_model*)(uintptr_t)1 && fake_hip_live_allocations() == live - 1);
        fake_hip_fail("hipMalloc", 0);
        CHECK(dsdtm_klt_model_create(s.ctx, 96, 72, 3, &s.t[0].model) == DSDTM_OK);
        // flow
        const float pts[4] = {40, 30, 20, 20};
        float out[4];
        dsdtm_klt_flow_desc f{};
        f.prev = (const uint8_t*)s.t[1].img[0].p; f.cur = (const uint8_t*)s.t[1].img[1].p; f.width = 96; f.height = 72; f.prev_stride = f.cur_stride = s.t[1].stride;
        f.n_points = 2; f.levels = 2; f.points = pts; f.out_points = out;
        for (Inject in : {Inject{"hipMemcpyAsync", 1}, Inject{nullptr, 1}, Inject{"pyrdown_launch", 2}, Inject{nullptr, 2}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 3}}) {
            fill_a5(out, sizeof out);
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_klt_fail(in.nth);
            const int rc = dsdtm_klt_flow(s.ctx, 1, &f);
            if (in.api) fake_hip_fail(in.api, 0); else fake_klt_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && all_a5(out, sizeof out) && fake_hip_pending() == 0);
        }
        CHECK(dsdtm_klt_flow(s.ctx, 1, &f) == DSDTM_OK && !all_a5(out, sizeof out));
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() { return addon_create_failures("dsdtm_amd_klt", dsdtm_klt_create, dsdtm_klt_destroy, dsdtm_klt_last_error); }

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"answers_and_memory_kinds", answers_and_memory_kinds}, {"refusals", refusals},
                                                      {"call_failures", call_failures}, {"create_failures", create_failures}};
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
