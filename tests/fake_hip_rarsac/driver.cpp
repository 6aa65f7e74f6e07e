// libdsdtm_amd_rarsac.so's host side (dsdtm_amd/csrc/rarsac_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified): the
// context, every refusal, the sort by bin and the tables, the packing of n problems into one block, the one upload / one launch / one
// read-back, every failure path — as a stand-alone program under ASan/UBSan/LSan. The launch is the fake of
// tests/fake_hip_rarsac/fake_rarsac.cpp. Test infrastructure (tests/test_rarsac_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_rarsac.h"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_rarsac.h"

// one problem: exactly-sized point arrays (an over-read is ASan's), outputs prefilled with 0xA5
struct Problem {
    int m = 0;
    bool one_bin = false;
    std::vector<float> cur, prev, F;
    std::vector<uint8_t> status;
    dsdtm_rarsac_desc d{};
    void init(int m_, bool want_status = true, bool one_bin_ = false) {
        m = m_; one_bin = one_bin_;
        cur.resize(2 * (size_t)m); prev.resize(2 * (size_t)m);
        for (int i = 0; i < m; ++i) {
            cur[2 * i] = one_bin ? 5.0f + (float)(i % 7) : (float)((i * 97 + m) % 620) + 5.25f;
            cur[2 * i + 1] = one_bin ? 6.0f + (float)(i % 5) : (float)((i * 131 + 7) % 460) + 5.5f;
            prev[2 * i] = (float)((i * 41 + 3) % 630) + 1.0f;
            prev[2 * i + 1] = (float)((i * 59 + 11) % 470) + 1.0f;
        }
        F.assign(9, 0.0f);
        for (int j = 0; j < 9; ++j) F[j] = 0.5f + (float)j;
        status.assign(want_status ? (size_t)m + 5 : 0, 0xA5);
        memset(&d, 0, sizeof d);
        d.cur = cur.data(); d.prev = prev.data(); d.status = want_status ? status.data() : nullptr; d.F = F.data(); d.m = m;
        d.width = 640; d.height = 480;
        for (int j = 0; j < DSDTM_RARSAC_GRID; ++j) d.grid_probability_in[j] = 0.2 + 0.005 * j;
    }
    int bin(int i) const { return (int)(cur[2 * i + 1] / 64.0f) * 10 + (int)(cur[2 * i] / 48.0f); }
};

struct Batch {
    std::vector<Problem> p;
    std::vector<dsdtm_rarsac_desc> d;
    std::vector<dsdtm_rarsac_result> r;
    bool check = false;
    explicit Batch(std::initializer_list<int> ms) {
        p.resize(ms.size());
        size_t k = 0;
        for (int m : ms) { p[k].init(m < 0 ? -m : m, k % 3 != 2, m < 0); ++k; }          // a negative size: every point in one bin
        r.resize(p.size());
        sync();
        prefill();
    }
    void sync() { d.clear(); for (auto& x : p) d.push_back(x.d); }
    void prefill() {
        fill_a5(r.data(), r.size() * sizeof r[0]);
        for (auto& x : p) fill_a5(x.status.data(), x.status.size());
    }
    bool untouched() const {
        if (!all_a5(r.data(), r.size() * sizeof r[0])) return false;
        for (auto& x : p) if (!all_a5(x.status.data(), x.status.size())) return false;
        return true;
    }
    int run(dsdtm_rarsac_ctx* ctx) {
        sync();
        return check ? dsdtm_rarsac_check(ctx, (int)d.size(), d.data(), r.data()) : dsdtm_rarsac_reject_batch(ctx, (int)d.size(), d.data(), r.data());
    }
    // what the fake launch leaves (fake_rarsac.cpp); a problem with found = 0 keeps everything but `found`
    bool answered() const {
        for (size_t k = 0; k < p.size(); ++k) {
            const Problem& x = p[k];
            const dsdtm_rarsac_result& o = r[k];
            int distinct = 0;
            {
                bool seen[DSDTM_RARSAC_GRID] = {false};
                for (int i = 0; i < x.m; ++i) { if (!seen[x.bin(i)]) ++distinct; seen[x.bin(i)] = true; }
            }
            CHECK(x.one_bin == (distinct < 8));
            if (distinct < 8 && !check) {
                dsdtm_rarsac_result want;
                fill_a5(&want, sizeof want);
                want.found = 0;
                CHECK(memcmp(&want, &o, sizeof o) == 0 && all_a5(x.status.data(), x.status.size()));
                continue;
            }
            double sum = 0, prior_sum = 0;
            int count[DSDTM_RARSAC_GRID] = {0};
            // the fake sums the SORTED array: bin after bin, a bin's correspondences in index order
            for (int i = 0; i < x.m; ++i) count[x.bin(i)]++;
            for (int j = 0; j < DSDTM_RARSAC_GRID; ++j)
                for (int i = 0; i < x.m; ++i)
                    if (x.bin(i) == j) { sum += (double)x.cur[2 * i]; sum += (double)x.cur[2 * i + 1]; sum += (double)x.prev[2 * i]; sum += (double)x.prev[2 * i + 1]; }
            for (int j = 0; j < DSDTM_RARSAC_GRID; ++j) prior_sum = prior_sum + (check ? 0.5 : x.d.grid_probability_in[j]);
            const int iters = x.d.max_iterations > 0 ? x.d.max_iterations : DSDTM_RARSAC_DEFAULT_ITERATIONS;
            const double term = x.d.terminate_threshold > 0 ? x.d.terminate_threshold : DSDTM_RARSAC_DEFAULT_TERMINATE;
            CHECK(o.found == 1 && o.n_inliers == x.m && o.iterations_run == (check ? 0 : iters) && o.score == (check ? (double)x.F[0] : term));
            CHECK(o.best_hypothesis == (int)((x.d.seed ? x.d.seed : DSDTM_RARSAC_DEFAULT_SEED) & 0xFFFFu));
            for (int j = 0; j < 9; ++j) CHECK(o.F[j] == (check ? x.F[j] : (float)(sum + j)));
            for (int j = 0; j < DSDTM_RARSAC_GRID; ++j) CHECK(o.grid_probability_out[j] == (check ? 0.5 : x.d.grid_probability_in[j]) / prior_sum + (double)count[j]);
            if (!x.status.empty() && x.d.status) {
                for (int i = 0; i < x.m; ++i) CHECK(x.status[i] == (x.cur[2 * i] >= x.prev[2 * i] ? 1 : 0));          // back in the caller's order
                CHECK(all_a5(x.status.data() + x.m, 5));
            }
        }
        return true;
    }
};

// the copies, the launch and the wait of a call failing once (and the allocations of a staging block that must grow): an error, every
// output untouched, nothing pending, nothing leaked; the next call succeeds
static bool call_failures() {
    dsdtm_rarsac_ctx* ctx = nullptr;
    CHECK(dsdtm_rarsac_create(0, &ctx) == DSDTM_OK);
    for (int pass = 0; pass < 2; ++pass) {
        Batch s{200, 8, -40, 64, 2048};
        s.check = pass == 1;
        CHECK(s.run(ctx) == DSDTM_OK && s.answered());
        s.prefill();
        const size_t live0 = fake_hip_live_allocations();
        auto failed_cleanly = [&](int rc) {
            CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_rarsac_last_error(ctx)) > 0 && s.untouched());
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
        fake_rarsac_fail(1);                                    // the launch
        const int rc = s.run(ctx);
        fake_rarsac_fail(0);
        CHECK(failed_cleanly(rc));
        CHECK(fake_hip_live_allocations() == live0);
    }
    // the single entry is the batch entry with n = 1
    Batch s{200};
    dsdtm_rarsac_result one;
    fill_a5(&one, sizeof one);
    fake_hip_fail("hipMemcpyAsync", 1);
    CHECK(dsdtm_rarsac_reject(ctx, 200, s.p[0].cur.data(), s.p[0].prev.data(), 640, 480, nullptr, s.p[0].status.data(), &one) == DSDTM_ERR_HIP);
    fake_hip_fail("hipMemcpyAsync", 0);
    CHECK(all_a5(&one, sizeof one) && s.untouched() && fake_hip_pending() == 0);
    CHECK(dsdtm_rarsac_reject(ctx, 200, s.p[0].cur.data(), s.p[0].prev.data(), 640, 480, nullptr, s.p[0].status.data(), &one) == DSDTM_OK && one.found == 1 &&
          one.n_inliers == 200 && one.iterations_run == DSDTM_RARSAC_DEFAULT_ITERATIONS && one.grid_probability_out[99] == 0.01);
    // a fresh context whose staging block cannot be had: pinned, then device
    for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
        dsdtm_rarsac_ctx* c2 = nullptr;
        CHECK(dsdtm_rarsac_create(0, &c2) == DSDTM_OK);
        Batch q{64, 9};
        fake_hip_fail(api, 1);
        const int rc2 = q.run(c2);
        fake_hip_fail(api, 0);
        CHECK(rc2 == DSDTM_ERR_HIP && q.untouched() && fake_hip_pending() == 0);
        CHECK(q.run(c2) == DSDTM_OK && q.answered());
        dsdtm_rarsac_destroy(c2);
    }
    dsdtm_rarsac_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool expect_invalid(dsdtm_rarsac_ctx* ctx, Batch& s, const char* index, const char* what) {
    const long l0 = fake_rarsac_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    const int rc = s.run(ctx);
    const char* e = dsdtm_rarsac_last_error(ctx);
    if (rc != DSDTM_ERR_INVALID || !s.untouched() || !strstr(e, what) || !strstr(e, index) || fake_rarsac_launches() != l0 || fake_hip_calls("hipMemcpyAsync") != c0) {
        std::fprintf(stderr, "expected INVALID naming '%s' and '%s': rc %d, error '%s'\n", index, what, rc, e);
        return false;
    }
    std::printf("ok refusal: %s\n", what);
    return true;
}

// n = 0; n over its limit; ONE launch, one upload and one read-back for a batch; the full batch
static bool batch_rules() {
    dsdtm_rarsac_ctx* ctx = nullptr;
    CHECK(dsdtm_rarsac_create(0, &ctx) == DSDTM_OK);
    const long l0 = fake_rarsac_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    dsdtm_rarsac_result none;
    CHECK(dsdtm_rarsac_reject_batch(ctx, 0, nullptr, nullptr) == DSDTM_OK && dsdtm_rarsac_check(ctx, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(fake_rarsac_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);          // nothing done
    CHECK(dsdtm_rarsac_reject_batch(ctx, -1, nullptr, &none) == DSDTM_ERR_INVALID && dsdtm_rarsac_reject_batch(nullptr, 0, nullptr, nullptr) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_rarsac_check(nullptr, 0, nullptr, nullptr) == DSDTM_ERR_INVALID);
    Batch s{8, 64, 65, 257, 2048, 40, -12};
    CHECK(dsdtm_rarsac_reject_batch(ctx, 3, nullptr, s.r.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_rarsac_last_error(ctx), "descs"));
    s.sync();
    CHECK(dsdtm_rarsac_reject_batch(ctx, 3, s.d.data(), nullptr) == DSDTM_ERR_INVALID && strstr(dsdtm_rarsac_last_error(ctx), "results"));
    const long s0 = fake_hip_calls("hipStreamSynchronize");
    CHECK(s.run(ctx) == DSDTM_OK && s.answered());
    CHECK(fake_rarsac_launches() == l0 + 1 && fake_hip_calls("hipMemcpyAsync") == c0 + 2);
    CHECK(fake_hip_calls("hipStreamSynchronize") == s0 + 2);          // the fake launch's drain and the call's one wait
    s.prefill();
    std::vector<dsdtm_rarsac_desc> big((size_t)DSDTM_RARSAC_MAX_PROBLEMS + 1, s.d[0]);
    std::vector<dsdtm_rarsac_result> big_r(big.size());
    CHECK(dsdtm_rarsac_reject_batch(ctx, (int)big.size(), big.data(), big_r.data()) == DSDTM_ERR_INVALID && strstr(dsdtm_rarsac_last_error(ctx), "n ="));
    std::vector<dsdtm_rarsac_desc> full((size_t)DSDTM_RARSAC_MAX_PROBLEMS, s.p[0].d);
    std::vector<dsdtm_rarsac_result> full_r(full.size());
    for (auto& d : full) d.status = nullptr;
    CHECK(dsdtm_rarsac_reject_batch(ctx, (int)full.size(), full.data(), full_r.data()) == DSDTM_OK);
    for (auto& o : full_r) CHECK(o.found == 1 && o.n_inliers == 8);
    dsdtm_rarsac_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// every refusal, each naming the problem and the field (and the index where there is one), for both entries
static bool refusals() {
    dsdtm_rarsac_ctx* ctx = nullptr;
    CHECK(dsdtm_rarsac_create(0, &ctx) == DSDTM_OK);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int pass = 0; pass < 2; ++pass) {
        Batch s{30, 120};
        s.check = pass == 1;
        const dsdtm_rarsac_desc good = s.p[1].d;
        auto& d = s.p[1].d;
        d.m = 7; CHECK(expect_invalid(ctx, s, "problem 1", "m out of range")); d = good;
        d.m = DSDTM_RARSAC_MAX_POINTS + 1; CHECK(expect_invalid(ctx, s, "problem 1", "m out of range")); d = good;
        d.cur = nullptr; CHECK(expect_invalid(ctx, s, "problem 1", "cur is NULL")); d = good;
        d.prev = nullptr; CHECK(expect_invalid(ctx, s, "problem 1", "prev is NULL")); d = good;
        d.width = 9; CHECK(expect_invalid(ctx, s, "problem 1", "width out of range")); d = good;
        d.height = DSDTM_RARSAC_MAX_SIDE + 1; CHECK(expect_invalid(ctx, s, "problem 1", "height out of range")); d = good;
        d.sigma = nan; CHECK(expect_invalid(ctx, s, "problem 1", "sigma")); d = good;
        d.sigma = -1.0f; CHECK(expect_invalid(ctx, s, "problem 1", "sigma")); d = good;
        s.p[1].cur[2 * 100 + 1] = nan; CHECK(expect_invalid(ctx, s, "problem 1", "cur is not finite at index 100")); s.p[1].cur[2 * 100 + 1] = 9.0f;
        s.p[1].prev[2 * 64] = inf; CHECK(expect_invalid(ctx, s, "problem 1", "prev is not finite at index 64")); s.p[1].prev[2 * 64] = 2.0f;
        const float keep = s.p[1].cur[2 * 17 + 1];
        s.p[1].cur[2 * 17 + 1] = 640.0f;          // row 10 of a 640 x 480 frame: bin 100 and up
        CHECK(expect_invalid(ctx, s, "problem 1", "cur lies outside the 10x10 grid (R1) at index 17"));
        s.p[1].cur[2 * 17 + 1] = -140.0f;         // row -2, column 11: bin -9
        CHECK(expect_invalid(ctx, s, "problem 1", "(R1) at index 17"));
        s.p[1].cur[2 * 17 + 1] = 3.0e30f;         // a quotient no int holds
        CHECK(expect_invalid(ctx, s, "problem 1", "(R1) at index 17"));
        s.p[1].cur[2 * 17 + 1] = keep;
        if (s.check) {
            d.F = nullptr; CHECK(expect_invalid(ctx, s, "problem 1", "F is NULL")); d = good;
            s.p[1].F[4] = nan; CHECK(expect_invalid(ctx, s, "problem 1", "F is not finite at entry 4")); s.p[1].F[4] = 1.0f;
        } else {
            d.max_iterations = -1; CHECK(expect_invalid(ctx, s, "problem 1", "max_iterations out of range")); d = good;
            d.max_iterations = DSDTM_RARSAC_MAX_ITERATIONS + 1; CHECK(expect_invalid(ctx, s, "problem 1", "max_iterations out of range")); d = good;
            d.terminate_threshold = std::numeric_limits<double>::quiet_NaN(); CHECK(expect_invalid(ctx, s, "problem 1", "terminate_threshold")); d = good;
            d.terminate_threshold = -0.5; CHECK(expect_invalid(ctx, s, "problem 1", "terminate_threshold")); d = good;
            d.grid_probability_in[33] = 1.5; CHECK(expect_invalid(ctx, s, "problem 1", "grid_probability_in outside 0..1 at bin 33")); d = good;
            d.grid_probability_in[7] = std::numeric_limits<double>::quiet_NaN(); CHECK(expect_invalid(ctx, s, "problem 1", "at bin 7")); d = good;
            for (int j = 0; j < DSDTM_RARSAC_GRID; ++j) d.grid_probability_in[j] = 0.0;
            CHECK(expect_invalid(ctx, s, "problem 1", "grid_probability_in sums to 0")); d = good;
        }
        s.p[0].d.m = 3; CHECK(expect_invalid(ctx, s, "problem 0", "m out of range")); s.p[0].d.m = 30;
        // zero means the defaults; other values reach the kernel's record; a status nobody asked for stays alone
        CHECK(s.run(ctx) == DSDTM_OK && s.answered());
        s.prefill();
        d.max_iterations = 257; d.terminate_threshold = 0.25; d.seed = 77u; d.sigma = 1.0f; d.status = nullptr;
        CHECK(s.run(ctx) == DSDTM_OK && s.answered() && s.r[1].best_hypothesis == 77 && all_a5(s.p[1].status.data(), s.p[1].status.size()));
        d = good;
    }
    // the single entry
    Batch s{30};
    dsdtm_rarsac_result one;
    fill_a5(&one, sizeof one);
    CHECK(dsdtm_rarsac_reject(ctx, 30, nullptr, s.p[0].prev.data(), 640, 480, nullptr, nullptr, &one) == DSDTM_ERR_INVALID && strstr(dsdtm_rarsac_last_error(ctx), "problem 0: cur"));
    CHECK(dsdtm_rarsac_reject(ctx, 30, s.p[0].cur.data(), s.p[0].prev.data(), 640, 480, nullptr, nullptr, nullptr) == DSDTM_ERR_INVALID && all_a5(&one, sizeof one));
    CHECK(dsdtm_rarsac_reject(nullptr, 30, s.p[0].cur.data(), s.p[0].prev.data(), 640, 480, nullptr, nullptr, &one) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_rarsac_reject(ctx, 7, s.p[0].cur.data(), s.p[0].prev.data(), 640, 480, nullptr, nullptr, &one) == DSDTM_ERR_INVALID && all_a5(&one, sizeof one));
    Batch q{-20};
    CHECK(dsdtm_rarsac_reject(ctx, 20, q.p[0].cur.data(), q.p[0].prev.data(), 640, 480, nullptr, q.p[0].status.data(), &one) == DSDTM_OK && one.found == 0 &&
          one.n_inliers == (int32_t)0xA5A5A5A5 && q.untouched());
    dsdtm_rarsac_destroy(ctx);
    dsdtm_rarsac_destroy(nullptr);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_rarsac", dsdtm_rarsac_create, dsdtm_rarsac_destroy, dsdtm_rarsac_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"call_failures", call_failures}, {"batch_rules", batch_rules}, {"refusals", refusals},
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
