// libdsdtm_amd_framediff.so's host side (dsdtm_amd/csrc/framediff_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified):
// a batch of mixed sizes with a, b, mask and warped in pageable, pinned and device memory, b = a, a mask nobody asked for, the batch against
// the single entry, the warp entry, every refusal (one scenario line each inside `refusals`), every HIP call and launch failing in turn —
// as a stand-alone program under ASan/UBSan/LSan. The launches are the fakes of fake_framediff.cpp.
// Test infrastructure (tests/test_framediff_cpu.py); nothing here is part of the product.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_framediff.h"
#include "../../dsdtm_amd/host/dsdtm_framediff_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_framediff.h"

enum Mem { PAGEABLE, PINNED, DEVICE };

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
    uint8_t* u8() const { return (uint8_t*)p; }
};

// one pair: images of exactly (h - 1) stride + w bytes, outputs prefilled with 0xA5
struct Pair {
    int w = 0, h = 0, sa = 0, sb = 0, sm = 0, sw = 0, nf = 0;
    bool same = false, want_mask = true, want_warped = false;
    Buf a, b, mask, warped;
    double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int flags = 0, threshold = 30, maxval = 255;
    std::vector<float> feat;
    std::vector<uint8_t> on;
    size_t bytes(int stride) const { return (size_t)(h - 1) * stride + w; }
    bool init(int w_, int h_, Mem in, Mem out, int pad, int seed, bool same_, bool want_mask_, bool want_warped_, int nf_) {
        w = w_; h = h_; sa = w + pad; sb = w + 2 * pad; sm = w + pad; sw = w + 3 * pad; same = same_; want_mask = want_mask_; want_warped = want_warped_; nf = nf_;
        if (same) sb = sa;
        CHECK(a.make(in, bytes(sa)) && (same || b.make(in, bytes(sb))));
        unsigned s = (unsigned)seed * 2654435761u + 1u;
        for (size_t i = 0; i < a.bytes; ++i) { s = s * 1664525u + 1013904223u; a.u8()[i] = (uint8_t)(s >> 24); }
        if (!same) for (size_t i = 0; i < b.bytes; ++i) { s = s * 1664525u + 1013904223u; b.u8()[i] = (uint8_t)((s >> 24) / 4); }
        for (int y = 6; y < h - 4; ++y) for (int x = 5; x < w / 2; ++x) a.u8()[(size_t)y * sa + x] = 250;          // a blob that survives F6
        if (want_mask) CHECK(mask.make(out, bytes(sm)));
        if (want_warped) CHECK(warped.make(out, bytes(sw)));
        H[2] = 1.25 + seed; H[5] = -0.5; H[1] = 0.01;
        feat.resize((size_t)nf * 2); on.resize((size_t)nf);
        for (int i = 0; i < nf; ++i) { feat[2 * (size_t)i] = (float)((i * 7) % w) + 0.5f; feat[2 * (size_t)i + 1] = (float)((i * 5) % h) - 0.25f; }
        prefill();
        return true;
    }
    void prefill() {
        if (mask.p) fill_a5(mask.p, mask.bytes);
        if (warped.p) fill_a5(warped.p, warped.bytes);
        fill_a5(on.data(), on.size());
    }
    bool untouched() const { return (!mask.p || all_a5(mask.p, mask.bytes)) && (!warped.p || all_a5(warped.p, warped.bytes)) && all_a5(on.data(), on.size()); }
    dsdtm_framediff_desc desc() {
        dsdtm_framediff_desc d{};
        d.a = a.u8(); d.b = same ? a.u8() : b.u8(); d.width = w; d.height = h; d.a_stride = sa; d.b_stride = sb;
        memcpy(d.H, H, sizeof H);
        d.flags = flags; d.threshold = threshold; d.maxval = maxval; d.mask = mask.u8(); d.mask_stride = sm; d.warped = warped.u8(); d.warped_stride = sw;
        d.n_features = nf; d.feature_px = nf ? feat.data() : nullptr; d.feature_on_mask = nf ? on.data() : nullptr;
        return d;
    }
    // every byte the call may write, by the host function; the gaps between rows stay 0xA5
    bool answered(const dsdtm_framediff_result& r) const {
        std::vector<uint8_t> m((size_t)w * h), f((size_t)nf);
        const uint8_t* bp = same ? a.u8() : b.u8();
        const DSDTM::FrameDiffHost want = DSDTM::frame_diff_host(a.u8(), sa, bp, sb, w, h, H, flags, threshold, maxval, m.data(), w, nf, feat.data(), f.data());
        CHECK(want.ok && memcmp(r.M, want.M, sizeof r.M) == 0 && r.n_foreground == want.n_foreground && r.n_flagged == want.n_flagged);
        CHECK(same || want.n_foreground > 0);
        for (int y = 0; y < h; ++y) {
            if (mask.p) CHECK(memcmp(mask.u8() + (size_t)y * sm, m.data() + (size_t)y * w, (size_t)w) == 0 && (y == h - 1 || all_a5(mask.u8() + (size_t)y * sm + w, (size_t)(sm - w))));
            if (warped.p) CHECK(memcmp(warped.u8() + (size_t)y * sw, want.warped.data() + (size_t)y * w, (size_t)w) == 0 && (y == h - 1 || all_a5(warped.u8() + (size_t)y * sw + w, (size_t)(sw - w))));
        }
        CHECK(f == on);
        return true;
    }
};

struct World {
    dsdtm_framediff_ctx* ctx = nullptr;
    Pair p[5];
    std::vector<dsdtm_framediff_result> res;
    bool init() {
        CHECK(dsdtm_framediff_create(0, &ctx) == DSDTM_OK);
        // pageable in and out with odd strides, features; pinned in, device out, warped too; device in, pageable out; b = a (pageable);
        // no mask wanted but features (the scratch mask) and the inverse map
        CHECK(p[0].init(70, 37, PAGEABLE, PAGEABLE, 3, 1, false, true, true, 9) && p[1].init(129, 45, PINNED, DEVICE, 0, 2, false, true, true, 0) &&
              p[2].init(64, 16, DEVICE, PAGEABLE, 5, 3, false, true, false, 4) && p[3].init(96, 40, PAGEABLE, PINNED, 1, 4, true, true, false, 3) &&
              p[4].init(33, 21, PAGEABLE, PAGEABLE, 2, 5, false, false, false, 12));
        p[4].flags = DSDTM_FRAMEDIFF_INVERSE_MAP; p[2].maxval = 0;
        prefill();
        return true;
    }
    void prefill() { for (auto& x : p) x.prefill(); res.assign(5, dsdtm_framediff_result{}); fill_a5(res.data(), res.size() * sizeof(dsdtm_framediff_result)); }
    bool untouched() const { for (auto& x : p) if (!x.untouched()) return false; return all_a5(res.data(), res.size() * sizeof(dsdtm_framediff_result)); }
    std::vector<dsdtm_framediff_desc> descs() { std::vector<dsdtm_framediff_desc> d; for (auto& x : p) d.push_back(x.desc()); return d; }
    int run() {
        std::vector<dsdtm_framediff_desc> d = descs();
        const int rc = dsdtm_framediff_steps(ctx, 5, d.data(), res.data());
        if (rc != DSDTM_OK) std::fprintf(stderr, "steps: %d %s\n", rc, dsdtm_framediff_last_error(ctx));
        return rc;
    }
    ~World() { for (auto& x : p) { x.a.release(); x.b.release(); x.mask.release(); x.warped.release(); } dsdtm_framediff_destroy(ctx); }
};

static bool answers_and_memory_kinds() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run() == DSDTM_OK);
        for (int k = 0; k < 5; ++k) CHECK(s.p[k].answered(s.res[(size_t)k]));
        CHECK(s.res[2].n_flagged == 0);                          // maxval 0 is 200: QUIRK 2
        // again on the same context (the counters start at zero again), then every pair alone: bit-equal to its place in the batch
        const std::vector<dsdtm_framediff_result> batch = s.res;
        s.prefill();
        CHECK(s.run() == DSDTM_OK && memcmp(batch.data(), s.res.data(), batch.size() * sizeof(dsdtm_framediff_result)) == 0);
        for (int k = 0; k < 5; ++k) {
            s.p[k].prefill();
            dsdtm_framediff_desc d = s.p[k].desc();
            dsdtm_framediff_result one;
            CHECK(dsdtm_framediff_step(s.ctx, &d, &one) == DSDTM_OK && s.p[k].answered(one) && memcmp(&one, &batch[(size_t)k], sizeof one) == 0);
        }
        // the warp entry: a, mask and features are not read (they are poisoned here), warped required
        std::vector<dsdtm_framediff_desc> d = s.descs();
        dsdtm_framediff_desc wd[2] = {d[0], d[1]};
        for (auto& x : wd) { x.a = nullptr; x.mask = (uint8_t*)(uintptr_t)8; x.n_features = 1 << 30; x.threshold = -5; x.maxval = 999; }
        s.prefill();
        CHECK(dsdtm_framediff_warp(s.ctx, 2, wd) == DSDTM_OK);
        CHECK(all_a5(s.p[0].mask.p, s.p[0].mask.bytes) && all_a5(s.p[1].mask.p, s.p[1].mask.bytes));
        for (int k = 0; k < 2; ++k) {
            const Pair& p = s.p[k];
            double M[9];
            std::vector<uint8_t> want((size_t)p.w * p.h);
            CHECK(DSDTM::framediff_matrix_host(p.H, p.flags, M));
            DSDTM::warp_perspective_host(p.b.u8(), p.w, p.h, p.sb, M, want.data(), p.w);
            for (int y = 0; y < p.h; ++y) CHECK(memcmp(p.warped.u8() + (size_t)y * p.sw, want.data() + (size_t)y * p.w, (size_t)p.w) == 0);
        }
        CHECK(dsdtm_framediff_steps(s.ctx, 0, nullptr, nullptr) == DSDTM_OK && dsdtm_framediff_warp(s.ctx, 0, nullptr) == DSDTM_OK);
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every refusal leaves every output untouched and enqueues nothing
static bool refusals() {
    {
        World s;
        CHECK(s.init());
        auto refused = [&](std::vector<dsdtm_framediff_desc> d, int n, const char* needle, bool null_results = false) {
            s.prefill();
            const long launches = fake_framediff_launches();
            const int rc = dsdtm_framediff_steps(s.ctx, n, d.empty() ? nullptr : d.data(), null_results ? nullptr : s.res.data());
            CHECK(rc == DSDTM_ERR_INVALID && s.untouched() && fake_framediff_launches() == launches && fake_hip_pending() == 0);
            if (!strstr(dsdtm_framediff_last_error(s.ctx), needle)) std::fprintf(stderr, "message: %s (wanted: %s)\n", dsdtm_framediff_last_error(s.ctx), needle);
            CHECK(strstr(dsdtm_framediff_last_error(s.ctx), needle));
            std::printf("ok refusal: %s\n", needle);
            return true;
        };
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<dsdtm_framediff_desc> d = s.descs();
        CHECK(refused(d, -1, "outside 0..1024") && refused(d, DSDTM_FRAMEDIFF_MAX_STEPS + 1, "outside 0..1024") && refused({}, 5, "descs is NULL") &&
              refused(d, 5, "results is NULL", true));
        d = s.descs(); for (int k = 0; k < 9; ++k) d[0].H[k] = k + 1.0; CHECK(refused(d, 5, "desc 0: H is singular"));            // det of 1..9 is 0
        d = s.descs(); memset(d[1].H, 0, sizeof d[1].H); d[1].flags = 0; CHECK(refused(d, 5, "desc 1: H is singular"));
        d = s.descs(); d[0].H[4] = nan; CHECK(refused(d, 5, "desc 0: H is not finite"));
        d = s.descs(); d[4].H[8] = std::numeric_limits<double>::infinity(); CHECK(refused(d, 5, "desc 4: H is not finite"));      // (with the inverse map too)
        d = s.descs(); d[0].H[0] = 1e-300; d[0].H[4] = 1e-300; d[0].H[1] = 0; CHECK(refused(d, 5, "desc 0: H is singular or its inverse is not finite"));
        d = s.descs(); d[0].width = 15; CHECK(refused(d, 5, "desc 0: width out of range"));
        d = s.descs(); d[0].width = 4097; CHECK(refused(d, 5, "desc 0: width out of range"));
        d = s.descs(); d[0].height = 4097; CHECK(refused(d, 5, "desc 0: height out of range"));
        d = s.descs(); d[0].height = 8; CHECK(refused(d, 5, "desc 0: height out of range"));
        d = s.descs(); d[0].threshold = 255; CHECK(refused(d, 5, "desc 0: threshold outside 0..254"));
        d = s.descs(); d[0].threshold = -1; CHECK(refused(d, 5, "desc 0: threshold outside 0..254"));
        d = s.descs(); d[0].maxval = 256; CHECK(refused(d, 5, "desc 0: maxval outside 0..255"));
        d = s.descs(); d[0].maxval = -1; CHECK(refused(d, 5, "desc 0: maxval outside 0..255"));
        // a batch whose descs are fine up to a bad one at index k > 0: nothing of the good ones is written either
        d = s.descs(); d[3].threshold = 300; CHECK(refused(d, 5, "desc 3: threshold"));
        d = s.descs(); d[4].b = nullptr; CHECK(refused(d, 5, "desc 4: b is NULL"));
        d = s.descs(); d[2].a = nullptr; CHECK(refused(d, 5, "desc 2: a is NULL"));
        d = s.descs(); d[1].a_stride = d[1].width - 1; CHECK(refused(d, 5, "desc 1: a_stride"));
        d = s.descs(); d[1].b_stride = d[1].width - 1; CHECK(refused(d, 5, "desc 1: b_stride"));
        d = s.descs(); d[0].mask_stride = d[0].width - 1; CHECK(refused(d, 5, "desc 0: mask_stride"));
        d = s.descs(); d[0].warped_stride = 0; CHECK(refused(d, 5, "desc 0: warped_stride"));
        d = s.descs(); d[2].flags = 2; CHECK(refused(d, 5, "desc 2: flags"));
        d = s.descs(); d[0].n_features = DSDTM_FRAMEDIFF_MAX_FEATURES + 1; CHECK(refused(d, 5, "desc 0: n_features"));
        d = s.descs(); d[0].feature_px = nullptr; CHECK(refused(d, 5, "desc 0: feature_px is NULL"));
        d = s.descs(); d[0].feature_on_mask = nullptr; CHECK(refused(d, 5, "desc 0: feature_on_mask is NULL"));
        {
            std::vector<float> f = s.p[0].feat;
            d = s.descs(); d[0].feature_px = f.data();
            f[5] = std::numeric_limits<float>::infinity(); CHECK(refused(d, 5, "desc 0: feature_px is not finite at feature 2"));
            f[5] = 36.5f; CHECK(s.p[0].h == 37);                 // 36.5 rounds to 36: inside
            f[4] = 69.5f; CHECK(refused(d, 5, "desc 0: feature_px rounds outside the image at feature 2"));      // 69.5 rounds to 70
            f[4] = -0.6f; CHECK(refused(d, 5, "feature 2"));
        }
        d = s.descs(); d[0].mask = const_cast<uint8_t*>(d[0].a) + 10; CHECK(refused(d, 5, "desc 0: mask overlaps a of desc 0"));
        d = s.descs(); d[3].mask = d[0].mask; d[3].mask_stride = d[3].width; CHECK(refused(d, 5, "overlaps mask of desc"));
        d = s.descs(); d[0].warped = d[0].mask + 1; CHECK(refused(d, 5, "overlaps"));
        CHECK(dsdtm_framediff_steps(nullptr, 5, d.data(), s.res.data()) == DSDTM_ERR_INVALID);
        dsdtm_framediff_result one;
        fill_a5(&one, sizeof one);
        CHECK(dsdtm_framediff_step(s.ctx, nullptr, &one) == DSDTM_ERR_INVALID && all_a5(&one, sizeof one));
        // the warp entry
        d = s.descs(); d[2].warped = nullptr;
        s.prefill();
        CHECK(dsdtm_framediff_warp(s.ctx, 5, d.data()) == DSDTM_ERR_INVALID && s.untouched() && strstr(dsdtm_framediff_last_error(s.ctx), "desc 2: warped is NULL"));
        // nothing of this stands in the way of the next call
        s.prefill();
        CHECK(s.run() == DSDTM_OK);
        for (int k = 0; k < 5; ++k) CHECK(s.p[k].answered(s.res[(size_t)k]));
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

struct Inject { const char* api; long nth; };

// every HIP call and every launch of a call failing in turn: host outputs untouched, nothing pending, and the next call answers
static bool call_failures() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run() == DSDTM_OK);
        // the two fakes wait once each; the call's own wait is the third
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipHostGetDevicePointer", 1}, Inject{"hipMemcpyAsync", 1}, Inject{"hipMemcpyAsync", 2},
                          Inject{"hipStreamSynchronize", 3}, Inject{nullptr, 1}, Inject{nullptr, 2}}) {
            s.prefill();
            if (!in.api) fake_framediff_fail(in.nth); else fake_hip_fail(in.api, in.nth);
            const int rc = s.run();
            if (!in.api) fake_framediff_fail(0); else fake_hip_fail(in.api, 0);
            // (a device output behind a launch is undefined after DSDTM_ERR_HIP: pair 1's, so only the host outputs are held to 0xA5)
            bool host_untouched = all_a5(s.res.data(), s.res.size() * sizeof(dsdtm_framediff_result));
            for (int k : {0, 2, 3, 4}) host_untouched = host_untouched && s.p[k].untouched();
            CHECK(rc == DSDTM_ERR_HIP && host_untouched && fake_hip_pending() == 0 && strlen(dsdtm_framediff_last_error(s.ctx)) > 0);
        }
        // the staging blocks cannot grow: a fresh context, nothing enqueued
        for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
            dsdtm_framediff_ctx* keep = s.ctx;
            CHECK(dsdtm_framediff_create(0, &s.ctx) == DSDTM_OK);
            s.prefill();
            fake_hip_fail(api, 1);
            const int rc = s.run();
            fake_hip_fail(api, 0);
            CHECK(rc == DSDTM_ERR_HIP && s.untouched() && fake_hip_pending() == 0);
            dsdtm_framediff_destroy(s.ctx);
            s.ctx = keep;
        }
        s.prefill();
        CHECK(s.run() == DSDTM_OK);
        for (int k = 0; k < 5; ++k) CHECK(s.p[k].answered(s.res[(size_t)k]));
        // the warp entry
        std::vector<dsdtm_framediff_desc> d = s.descs();
        for (Inject in : {Inject{"hipMemcpyAsync", 1}, Inject{nullptr, 1}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 2}}) {
            s.p[0].prefill();
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_framediff_fail(in.nth);
            const int rc = dsdtm_framediff_warp(s.ctx, 1, d.data());
            if (in.api) fake_hip_fail(in.api, 0); else fake_framediff_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && s.p[0].untouched() && fake_hip_pending() == 0);
        }
        CHECK(dsdtm_framediff_warp(s.ctx, 1, d.data()) == DSDTM_OK && !s.p[0].untouched());
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() { return addon_create_failures("dsdtm_amd_framediff", dsdtm_framediff_create, dsdtm_framediff_destroy, dsdtm_framediff_last_error); }

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
