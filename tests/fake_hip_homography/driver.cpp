// libdsdtm_amd_homography.so's host side (dsdtm_amd/csrc/homography_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified):
// the context, the checks, the packing of n problems into one block, the one upload / one launch / one read-back, every failure
// path — as a stand-alone program under ASan/UBSan/LSan. The launch is the fake of tests/fake_hip_homography/fake_homography.cpp.
// Test infrastructure (tests/test_homography_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_homography.h"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_homography.h"

// one problem: exactly-sized point arrays (an over-read is ASan's), outputs prefilled with 0xA5
struct Problem {
    int m = 0;
    std::vector<float> a, b;
    std::vector<uint8_t> mask;
    dsdtm_homography_desc d{};
    void init(int m_, bool want_mask = true) {
        m = m_;
        a.resize(2 * (size_t)m); b.resize(2 * (size_t)m);
        for (int i = 0; i < 2 * m; ++i) { a[i] = (float)((i * 37 + m) % 101); b[i] = (float)((i * 53 + 7) % 103); }
        mask.assign(want_mask ? (size_t)m + 5 : 0, 0xA5);
        memset(&d, 0, sizeof d);
        d.points_a = m ? a.data() : nullptr; d.points_b = m ? b.data() : nullptr; d.mask = want_mask ? mask.data() : nullptr; d.m = m;
    }
};

struct Batch {
    std::vector<Problem> p;
    std::vector<dsdtm_homography_desc> d;
    std::vector<dsdtm_homography_result> r;
    explicit Batch(std::initializer_list<int> ms) {
        p.resize(ms.size());
        size_t k = 0;
        for (int m : ms) { p[k].init(m, k % 3 != 2); ++k; }
        r.resize(p.size());
        sync();
        prefill();
    }
    void sync() { d.clear(); for (auto& x : p) d.push_back(x.d); }
    void prefill() {
        fill_a5(r.data(), r.size() * sizeof r[0]);
        for (auto& x : p) fill_a5(x.mask.data(), x.mask.size());
    }
    bool untouched() const {
        if (!all_a5(r.data(), r.size() * sizeof r[0])) return false;
        for (auto& x : p) if (!all_a5(x.mask.data(), x.mask.size())) return false;
        return true;
    }
    int run(dsdtm_homography_ctx* ctx) { sync(); return dsdtm_find_homographies(ctx, (int)d.size(), d.data(), r.data()); }
    // what the fake launch leaves (fake_homography.cpp); a problem with found = 0 keeps everything but `found`
    bool answered() const {
        for (size_t k = 0; k < p.size(); ++k) {
            const Problem& x = p[k];
            const dsdtm_homography_result& o = r[k];
            if (x.m <= 4) {
                dsdtm_homography_result want;
                fill_a5(&want, sizeof want);
                want.found = 0;
                CHECK(memcmp(&want, &o, sizeof o) == 0 && all_a5(x.mask.data(), x.mask.size()));
                continue;
            }
            double sum = 0;
            for (float v : x.a) sum += (double)v;
            const double thr = x.d.reproj_threshold > 0 ? x.d.reproj_threshold : 3.0, conf = x.d.confidence > 0 ? x.d.confidence : 0.995;
            const int hyp = x.d.max_hypotheses > 0 ? x.d.max_hypotheses : 2048;
            CHECK(o.found == 1 && o.n_inliers == x.m && o.rounds == (hyp + 255) / 256 && o.cost_before == thr * thr && o.cost_after == 1.0 - conf);
            CHECK(o.best_hypothesis == (int)((x.d.seed ? x.d.seed : DSDTM_HOMOGRAPHY_DEFAULT_SEED) & 0xFFFFu));
            for (int j = 0; j < 9; ++j) CHECK(o.H[j] == sum + j);
            if (!x.mask.empty()) {
                for (int i = 0; i < x.m; ++i) CHECK(x.mask[i] == (x.a[2 * i] >= x.b[2 * i] ? 1 : 0));
                CHECK(all_a5(x.mask.data() + x.m, 5));
            }
        }
        return true;
    }
};

// the copies, the launch and the wait of a call failing once (and the allocations of a staging block that must grow): an error, every
// output untouched, nothing pending, nothing leaked; the next call succeeds
static bool call_failures() {
    dsdtm_homography_ctx* ctx = nullptr;
    CHECK(dsdtm_homography_create(0, &ctx) == DSDTM_OK);
    Batch s{200, 5, 3, 64, 0, 2048};
    CHECK(s.run(ctx) == DSDTM_OK && s.answered());
    s.prefill();
    const size_t live0 = fake_hip_live_allocations();
    auto failed_cleanly = [&](int rc) {
        CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_homography_last_error(ctx)) > 0 && s.untouched());
        CHECK(s.run(ctx) == DSDTM_OK && s.answered());
        s.prefill();
        return true;
    };
    for (long nth = 1; nth <= 2; ++nth) {                   // the upload, the read-back
        fake_hip_fail("hipMemcpyAsync", nth);
        const int rc = s.run(ctx);
        fake_hip_fail("hipMemcpyAsync", 0);
        CHECK(failed_cleanly(rc));
    }
    for (long nth = 1; nth <= 2; ++nth) {                   // the launch's drain, the wait
        fake_hip_fail("hipStreamSynchronize", nth);
        const int rc = s.run(ctx);
        fake_hip_fail("hipStreamSynchronize", 0);
        CHECK(failed_cleanly(rc));
    }
    fake_homography_fail(1);                                // the launch
    const int rc = s.run(ctx);
    fake_homography_fail(0);
    CHECK(failed_cleanly(rc));
    // the single entry is the batch entry with n = 1
    dsdtm_homography_result one;
    fill_a5(&one, sizeof one);
    fake_hip_fail("hipMemcpyAsync", 1);
    CHECK(dsdtm_find_homography(ctx, 200, s.p[0].a.data(), s.p[0].b.data(), s.p[0].mask.data(), &one) == DSDTM_ERR_HIP);
    fake_hip_fail("hipMemcpyAsync", 0);
    CHECK(all_a5(&one, sizeof one) && s.untouched());
    CHECK(dsdtm_find_homography(ctx, 200, s.p[0].a.data(), s.p[0].b.data(), s.p[0].mask.data(), &one) == DSDTM_OK && one.found == 1 && one.n_inliers == 200);
    CHECK(fake_hip_live_allocations() == live0);
    // a fresh context whose staging block cannot be had: pinned, then device
    for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
        dsdtm_homography_ctx* c2 = nullptr;
        CHECK(dsdtm_homography_create(0, &c2) == DSDTM_OK);
        Batch q{64, 9};
        fake_hip_fail(api, 1);
        const int rc2 = q.run(c2);
        fake_hip_fail(api, 0);
        CHECK(rc2 == DSDTM_ERR_HIP && q.untouched() && fake_hip_pending() == 0);
        CHECK(q.run(c2) == DSDTM_OK && q.answered());
        dsdtm_homography_destroy(c2);
    }
    dsdtm_homography_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool expect_invalid(dsdtm_homography_ctx* ctx, Batch& s, const char* index, const char* what) {
    const long l0 = fake_homography_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    const int rc = s.run(ctx);
    const char* e = dsdtm_homography_last_error(ctx);
    if (rc != DSDTM_ERR_INVALID || !s.untouched() || !strstr(e, what) || !strstr(e, index) || fake_homography_launches() != l0 ||
        fake_hip_calls("hipMemcpyAsync") != c0) {
        std::fprintf(stderr, "expected INVALID naming '%s' and '%s': rc %d, error '%s'\n", index, what, rc, e);
        return false;
    }
    return true;
}

// n = 0; n over its limit; ONE launch, one upload and one read-back for a batch; m over the cap; a NaN coordinate in the middle
static bool batch_rules() {
    dsdtm_homography_ctx* ctx = nullptr;
    CHECK(dsdtm_homography_create(0, &ctx) == DSDTM_OK);
    const long l0 = fake_homography_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    dsdtm_homography_result none;
    CHECK(dsdtm_find_homographies(ctx, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(fake_homography_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);          // nothing done
    CHECK(dsdtm_find_homographies(ctx, -1, nullptr, &none) == DSDTM_ERR_INVALID && dsdtm_find_homographies(nullptr, 0, nullptr, nullptr) == DSDTM_ERR_INVALID);
    Batch s{5, 64, 65, 257, 2048, 40, 4};
    CHECK(dsdtm_find_homographies(ctx, 3, nullptr, s.r.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_homography_last_error(ctx), "descs"));
    s.sync();
    CHECK(dsdtm_find_homographies(ctx, 3, s.d.data(), nullptr) == DSDTM_ERR_INVALID && strstr(dsdtm_homography_last_error(ctx), "results"));
    const long s0 = fake_hip_calls("hipStreamSynchronize");
    CHECK(s.run(ctx) == DSDTM_OK && s.answered());
    CHECK(fake_homography_launches() == l0 + 1 && fake_hip_calls("hipMemcpyAsync") == c0 + 2);
    CHECK(fake_hip_calls("hipStreamSynchronize") == s0 + 2);          // the fake launch's drain and the call's one wait
    s.prefill();
    std::vector<dsdtm_homography_desc> big((size_t)DSDTM_HOMOGRAPHY_MAX_PROBLEMS + 1, s.d[0]);
    std::vector<dsdtm_homography_result> big_r(big.size());
    CHECK(dsdtm_find_homographies(ctx, (int)big.size(), big.data(), big_r.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_homography_last_error(ctx), "n ="));
    s.p[4].d.m = DSDTM_HOMOGRAPHY_MAX_POINTS + 1;
    CHECK(expect_invalid(ctx, s, "problem 4", "m out of range"));
    s.p[4].d.m = 2048;
    s.p[3].a[2 * 100 + 1] = std::numeric_limits<float>::quiet_NaN();
    CHECK(expect_invalid(ctx, s, "problem 3", "points_a is not finite at index 100"));
    s.p[3].a[2 * 100 + 1] = 1.0f;
    s.p[2].b[2 * 64] = std::numeric_limits<float>::infinity();
    CHECK(expect_invalid(ctx, s, "problem 2", "points_b is not finite at index 64"));
    s.p[2].b[2 * 64] = 2.0f;
    CHECK(s.run(ctx) == DSDTM_OK && s.answered());
    // the full batch
    std::vector<dsdtm_homography_desc> full((size_t)DSDTM_HOMOGRAPHY_MAX_PROBLEMS, s.p[0].d);
    std::vector<dsdtm_homography_result> full_r(full.size());
    for (auto& d : full) d.mask = nullptr;
    CHECK(dsdtm_find_homographies(ctx, (int)full.size(), full.data(), full_r.data()) == DSDTM_OK);
    for (auto& o : full_r) CHECK(o.found == 1 && o.n_inliers == 5);
    dsdtm_homography_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool argument_checks() {
    dsdtm_homography_ctx* ctx = nullptr;
    CHECK(dsdtm_homography_create(0, &ctx) == DSDTM_OK);
    Batch s{30, 12};
    const dsdtm_homography_desc good = s.p[1].d;
    auto& d = s.p[1].d;
    d.m = -1; CHECK(expect_invalid(ctx, s, "problem 1", "m out of range")); d = good;
    d.points_a = nullptr; CHECK(expect_invalid(ctx, s, "problem 1", "points_a is NULL")); d = good;
    d.points_b = nullptr; CHECK(expect_invalid(ctx, s, "problem 1", "points_b is NULL")); d = good;
    d.reproj_threshold = std::numeric_limits<double>::quiet_NaN(); CHECK(expect_invalid(ctx, s, "problem 1", "reproj_threshold")); d = good;
    d.confidence = 1.0; CHECK(expect_invalid(ctx, s, "problem 1", "confidence")); d = good;
    d.confidence = std::numeric_limits<double>::infinity(); CHECK(expect_invalid(ctx, s, "problem 1", "confidence")); d = good;
    d.max_hypotheses = DSDTM_HOMOGRAPHY_MAX_HYPOTHESES + 1; CHECK(expect_invalid(ctx, s, "problem 1", "max_hypotheses")); d = good;
    // non-positive values and zero mean the defaults; others reach the kernel's record
    d.reproj_threshold = -2.0; d.confidence = -1.0; d.max_hypotheses = -5; d.seed = 0;
    CHECK(s.run(ctx) == DSDTM_OK && s.answered());
    s.prefill();
    d.reproj_threshold = 1.0; d.confidence = 0.5; d.max_hypotheses = 257; d.seed = 77u; d.mask = nullptr;
    CHECK(s.run(ctx) == DSDTM_OK && s.r[1].rounds == 2 && s.r[1].cost_before == 1.0 && s.r[1].cost_after == 0.5 && s.r[1].best_hypothesis == 77);
    CHECK(all_a5(s.p[1].mask.data(), s.p[1].mask.size()));          // a mask nobody asked for
    d = good;
    // the single entry
    dsdtm_homography_result one;
    fill_a5(&one, sizeof one);
    CHECK(dsdtm_find_homography(ctx, 30, nullptr, s.p[0].b.data(), nullptr, &one) == DSDTM_ERR_INVALID && strstr(dsdtm_homography_last_error(ctx), "problem 0: points_a"));
    CHECK(dsdtm_find_homography(ctx, 30, s.p[0].a.data(), s.p[0].b.data(), nullptr, nullptr) == DSDTM_ERR_INVALID && all_a5(&one, sizeof one));
    CHECK(dsdtm_find_homography(nullptr, 30, s.p[0].a.data(), s.p[0].b.data(), nullptr, &one) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_find_homography(ctx, 4, s.p[0].a.data(), s.p[0].b.data(), s.p[0].mask.data(), &one) == DSDTM_OK && one.found == 0 && one.n_inliers == (int32_t)0xA5A5A5A5);
    CHECK(dsdtm_find_homography(ctx, 0, nullptr, nullptr, nullptr, &one) == DSDTM_OK && one.found == 0);
    dsdtm_homography_destroy(ctx);
    dsdtm_homography_destroy(nullptr);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_homography", dsdtm_homography_create, dsdtm_homography_destroy, dsdtm_homography_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"call_failures", call_failures}, {"batch_rules", batch_rules},
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
