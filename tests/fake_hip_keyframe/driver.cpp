// dsdtm_need_keyframes against the fake HIP runtime of tests/fake_hip (unmodified): the host side of libdsdtm_amd_keyframe.so
// (dsdtm_amd/csrc/keyframe_api.cpp) — the context, the checks, the packing of n trackers into one blob, the one upload / one
// launch / one read-back, every failure path — under ASan/UBSan/LSan. The launch is the fake of
// tests/fake_hip_keyframe/fake_keyframe.cpp. Test infrastructure (tests/test_need_keyframes_fake_hip_cpu.py); nothing here is
// part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_keyframe.h"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_keyframe.h"

static const dsdtm_camera CAM{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
static dsdtm_keyframe_params params() { dsdtm_keyframe_params p{}; p.min_valid = 30; p.max_valid = 50; p.px_samples = 31; p.min_px_median = 40; p.min_rot = p.min_trans = 0.08; return p; }

struct Tracker {
    std::vector<double> Tc, Tk, pc, pk, cen;
    std::vector<uint8_t> bc, bk;
    dsdtm_keyframe_desc d{};
    void init(int id, int n_cur, int n_kf, int n_lkf, bool with_bad) {
        Tc = {1, 0, 0, 0.5 + id, 0, 1, 0, 0, 0, 0, 1, 0}; Tk = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25 * id};
        pc.resize(3 * (size_t)n_cur); pk.resize(3 * (size_t)n_kf); cen.resize(3 * (size_t)n_lkf);
        for (size_t i = 0; i < pc.size(); ++i) pc[i] = (double)((i * 7 + (size_t)id) % 13);
        for (size_t i = 0; i < pk.size(); ++i) pk[i] = (double)((i * 5 + (size_t)id) % 11);
        for (size_t i = 0; i < cen.size(); ++i) cen[i] = (double)((i + (size_t)id) % 3);
        bc.assign((size_t)n_cur, 0); bk.assign((size_t)n_kf, 0);
        for (size_t i = 0; i < bc.size(); i += 3) bc[i] = 1;
        for (size_t i = 0; i < bk.size(); i += 4) bk[i] = 1;
        d.T_cur_w = Tc.data(); d.T_kf_w = Tk.data(); d.n_valid = 100 + id;
        d.n_cur_points = n_cur; d.cur_p_world = pc.data(); d.cur_bad = with_bad ? bc.data() : nullptr;
        d.n_kf_points = n_kf; d.kf_p_world = pk.data(); d.kf_bad = with_bad ? bk.data() : nullptr;
        d.n_local_kf = n_lkf; d.local_kf_centre = cen.data();
    }
    bool answered(const dsdtm_keyframe_verdict& v) const {          // what the fake launch leaves (fake_keyframe.cpp)
        auto sum = [](const std::vector<double>& a) { double s = 0; for (double x : a) s += x; return s; };
        auto sum8 = [](const std::vector<uint8_t>& a) { double s = 0; for (uint8_t x : a) s += x; return s; };
        CHECK(v.need == d.n_valid && v.reason == 31 && v.n_px == d.n_kf_points && v.n_depth == d.n_cur_points && v.svo_kf == d.n_local_kf);
        CHECK(v.median_px == sum(pk) && v.median_depth == sum(pc) && v.trans == sum(cen));
        CHECK(v.min_depth == (d.cur_bad ? sum8(bc) : 0.0) + 1000.0 * (d.kf_bad ? sum8(bk) : 0.0));
        CHECK(v.rot == Tc[3] + Tk[11] + 512.0);
        return true;
    }
};

struct Batch {
    std::vector<Tracker> t;
    std::vector<dsdtm_keyframe_desc> d;
    std::vector<dsdtm_keyframe_verdict> v;
    void init(const std::vector<std::vector<int>>& shapes) {
        t.resize(shapes.size());
        for (size_t i = 0; i < shapes.size(); ++i) t[i].init((int)i, shapes[i][0], shapes[i][1], shapes[i][2], i % 2 == 0);
        refresh();
        v.resize(shapes.size());
        prefill();
    }
    void refresh() { d.clear(); for (auto& x : t) d.push_back(x.d); }
    void prefill() { fill_a5(v.data(), v.size() * sizeof(dsdtm_keyframe_verdict)); }
    bool untouched() const { return all_a5(v.data(), v.size() * sizeof(dsdtm_keyframe_verdict)); }
    int run(dsdtm_keyframe_ctx* ctx, const dsdtm_keyframe_params& p) { return dsdtm_need_keyframes(ctx, &CAM, &p, (int)d.size(), d.data(), v.data()); }
    bool answered() const { for (size_t i = 0; i < t.size(); ++i) if (!t[i].answered(v[i])) return false; return true; }
};

// the upload, the launch, the read-back and the wait each fail once (and the allocations of a staging block that must grow):
// an error, the verdicts untouched, nothing pending, nothing leaked; the context stays usable
static bool keyframe_failures() {
    dsdtm_keyframe_ctx* ctx = nullptr;
    CHECK(dsdtm_keyframe_create(0, &ctx) == DSDTM_OK);
    const dsdtm_keyframe_params p = params();
    Batch b;
    b.init({{200, 300, 10}, {0, 0, 0}, {1, 31, 1}, {65, 30, 64}, {4096, 4096, 64}});
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
    const size_t live0 = fake_hip_live_allocations();
    const char* points[] = {"hipMemcpyAsync", "hipStreamSynchronize"};
    for (const char* api : points)
        for (long nth = 1; nth <= 2; ++nth) {            // 1: the upload / the launch's drain; 2: the read-back / the wait
            b.prefill();
            fake_hip_fail(api, nth);
            const int rc = b.run(ctx, p);
            fake_hip_fail(api, 0);
            CHECK(rc == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0);
            CHECK(strlen(dsdtm_keyframe_last_error(ctx)) > 0);
            CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
        }
    b.prefill();
    fake_keyframe_fail(1);
    CHECK(b.run(ctx, p) == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0);
    fake_keyframe_fail(0);
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
    CHECK(fake_hip_live_allocations() == live0);
    dsdtm_keyframe_destroy(ctx);
    // a fresh context whose staging block cannot be had: pinned, then device
    for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
        CHECK(dsdtm_keyframe_create(0, &ctx) == DSDTM_OK);
        for (long nth = 1; nth <= 3; ++nth) {
            b.prefill();
            fake_hip_fail(api, nth);
            const int rc = b.run(ctx, p);
            fake_hip_fail(api, 0);
            if (rc == DSDTM_OK) { CHECK(b.answered()); continue; }      // (fewer than nth calls of this api)
            CHECK(b.untouched() && fake_hip_pending() == 0);
            CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
        }
        dsdtm_keyframe_destroy(ctx);
    }
    CHECK(fake_hip_errors().empty());
    return true;
}

// n at its limit; every count at its limit; one over each; the degenerate calls
static bool keyframe_limits() {
    dsdtm_keyframe_ctx* ctx = nullptr;
    CHECK(dsdtm_keyframe_create(0, &ctx) == DSDTM_OK);
    dsdtm_keyframe_params p = params();
    Batch b;
    std::vector<std::vector<int>> shapes;
    for (int i = 0; i < DSDTM_TRACK_FRAMES_MAX; ++i) shapes.push_back({i % 7, (i * 3) % 40, i % 5});
    shapes[1023] = {DSDTM_KF_MAX_POINTS, DSDTM_KF_MAX_POINTS, DSDTM_KF_MAX_LOCAL_KF};
    b.init(shapes);
    const long l0 = fake_keyframe_launches();
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered() && fake_keyframe_launches() == l0 + 1);      // ONE launch for 1024 trackers
    // n == 0: nothing done, nothing dereferenced
    CHECK(dsdtm_need_keyframes(ctx, &CAM, &p, 0, nullptr, nullptr) == DSDTM_OK && fake_keyframe_launches() == l0 + 1);
    // the single entry is the batch entry with n = 1
    dsdtm_keyframe_verdict one;
    CHECK(dsdtm_need_keyframe(ctx, &CAM, &p, &b.d[1023], &one) == DSDTM_OK && b.t[1023].answered(one));
    b.prefill();
    const long l1 = fake_keyframe_launches();
    auto invalid = [&](const char* what) {
        const int rc = b.run(ctx, p);
        if (rc != DSDTM_ERR_INVALID || !b.untouched() || !strstr(dsdtm_keyframe_last_error(ctx), what)) {
            std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_keyframe_last_error(ctx));
            return false;
        }
        return true;
    };
    CHECK(dsdtm_need_keyframes(ctx, &CAM, &p, DSDTM_TRACK_FRAMES_MAX + 1, b.d.data(), b.v.data()) == DSDTM_ERR_INVALID && b.untouched());
    CHECK(dsdtm_need_keyframes(ctx, &CAM, &p, -1, b.d.data(), b.v.data()) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_need_keyframes(ctx, nullptr, &p, 3, b.d.data(), b.v.data()) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_need_keyframes(ctx, &CAM, nullptr, 3, b.d.data(), b.v.data()) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_need_keyframes(ctx, &CAM, &p, 3, nullptr, b.v.data()) == DSDTM_ERR_INVALID);
    CHECK(dsdtm_need_keyframes(ctx, &CAM, &p, 3, b.d.data(), nullptr) == DSDTM_ERR_INVALID);
    p.px_samples = 0; CHECK(invalid("px_samples"));
    p.px_samples = 65; CHECK(invalid("px_samples"));
    p.px_samples = 64; CHECK(b.run(ctx, p) == DSDTM_OK); b.prefill();
    p.px_samples = 31;
    b.d[7].n_cur_points = DSDTM_KF_MAX_POINTS + 1; CHECK(invalid("tracker 7: n_cur_points")); b.refresh();
    b.d[8].n_kf_points = DSDTM_KF_MAX_POINTS + 1; CHECK(invalid("tracker 8: n_kf_points")); b.refresh();
    b.d[9].n_local_kf = DSDTM_KF_MAX_LOCAL_KF + 1; CHECK(invalid("tracker 9: n_local_kf")); b.refresh();
    b.d[9].n_local_kf = -1; CHECK(invalid("tracker 9: n_local_kf")); b.refresh();
    b.d[1023].cur_p_world = nullptr; CHECK(invalid("tracker 1023: cur_p_world")); b.refresh();
    b.d[1023].kf_p_world = nullptr; CHECK(invalid("tracker 1023: kf_p_world")); b.refresh();
    b.d[1023].local_kf_centre = nullptr; CHECK(invalid("tracker 1023: local_kf_centre")); b.refresh();
    b.d[5].T_cur_w = nullptr; CHECK(invalid("tracker 5: T_cur_w")); b.refresh();
    b.d[5].T_kf_w = nullptr; CHECK(invalid("tracker 5: T_kf_w")); b.refresh();
    // a NULL array with a zero count is fine
    b.d[0].cur_p_world = nullptr; b.d[0].kf_p_world = nullptr; b.d[0].local_kf_centre = nullptr;
    CHECK(b.d[0].n_cur_points == 0 && b.d[0].n_kf_points == 0 && b.d[0].n_local_kf == 0);
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
    CHECK(fake_keyframe_launches() == l1 + 2);            // (px_samples = 64 and this one: no refused call reached the launch)
    dsdtm_keyframe_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// a descriptor rejected in the middle of a batch: a non-finite pose entry, world point or camera centre (the host scan) —
// the tracker and the field are named, nothing was enqueued, the verdicts of ALL trackers are untouched
static bool rejected_in_the_middle() {
    dsdtm_keyframe_ctx* ctx = nullptr;
    CHECK(dsdtm_keyframe_create(0, &ctx) == DSDTM_OK);
    const dsdtm_keyframe_params p = params();
    Batch b;
    b.init({{20, 40, 3}, {30, 35, 2}, {63, 31, 5}, {64, 32, 1}, {9, 9, 9}});
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
    b.prefill();
    const long l0 = fake_keyframe_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    struct Poke { std::vector<double>* v; size_t at; double bad; const char* what; };
    const Poke pokes[] = {{&b.t[2].pk, 3 * 30 + 1, nan, "tracker 2: kf_p_world"}, {&b.t[2].pc, 3 * 62 + 2, inf, "tracker 2: cur_p_world"},
                          {&b.t[2].cen, 14, -inf, "tracker 2: local_kf_centre"}, {&b.t[3].Tc, 11, nan, "tracker 3: T_cur_w"},
                          {&b.t[1].Tk, 0, inf, "tracker 1: T_kf_w"}};
    for (const Poke& k : pokes) {
        const double keep = (*k.v)[k.at];
        (*k.v)[k.at] = k.bad;
        CHECK(b.run(ctx, p) == DSDTM_ERR_INVALID && b.untouched() && strstr(dsdtm_keyframe_last_error(ctx), k.what) != nullptr);
        (*k.v)[k.at] = keep;
    }
    CHECK(fake_keyframe_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0 && fake_hip_pending() == 0);   // nothing was enqueued
    // a bad point's coordinates are scanned too (the flag does not excuse a NaN), and the batch works again afterwards
    b.t[0].pk[0] = nan;
    CHECK(b.t[0].bk[0] == 1 && b.run(ctx, p) == DSDTM_ERR_INVALID && b.untouched());
    b.t[0].pk[0] = 0.0;
    CHECK(b.run(ctx, p) == DSDTM_OK && b.answered());
    dsdtm_keyframe_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_keyframe", dsdtm_keyframe_create, dsdtm_keyframe_destroy, dsdtm_keyframe_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"keyframe_failures", keyframe_failures}, {"keyframe_limits", keyframe_limits},
                                                      {"rejected_in_the_middle", rejected_in_the_middle}, {"create_failures", create_failures}};
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
