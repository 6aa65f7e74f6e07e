// libdsdtm_amd_slam.so's host side (dsdtm_amd/csrc/slam_api.cpp over trackmap_api_body.h and mapping_api_body.h) against the fake HIP
// runtime of tests/fake_hip (unmodified): the checks and the packing of dsdtm_slam_track_commit — the grouping of descs by map, every
// refusal, every failing HIP call, the growth of the staging blocks — and the map and mapping entries under their dsdtm_slam_* names,
// under ASan/UBSan/LSan. The launch of aftertrack.hip is the fake of tests/fake_hip_slam/fake_slam.cpp (track_commit_host of
// dsdtm_slam_host.hpp), the others those of tests/fake_hip_mapping, tests/fake_hip_trackmap and tests/fake_hip_localmap. Test
// infrastructure (tests/test_aftertrack_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_mapping_host.hpp"
#include "../../dsdtm_amd/host/dsdtm_slam_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_keyframe.h"
#include "fake_mapping.h"
#include "fake_slam.h"
#include "fake_trackmap.h"

static const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static const double THR = 0.5;

static bool named_err(dsdtm_slam_ctx* ctx, int rc, const char* needle) {
    if (rc != DSDTM_ERR_INVALID || !strstr(dsdtm_slam_last_error(ctx), needle)) {
        std::fprintf(stderr, "rc %d, error \"%s\", wanted \"%s\"\n", rc, dsdtm_slam_last_error(ctx), needle);
        return false;
    }
    return true;
}

// A map on the "device" and its mirror on the host: K keyframes of S slots; slot s of keyframe k lists point (k * stride + s) % P and
// observes it unless (k + s) % 5 == 0; point i has the found count i % 3 (every third one goes bad when it is erased).
struct World {
    dsdtm_slam_ctx* ctx = nullptr;
    bool own_ctx = true;
    dsdtm_trackmap* map = nullptr;
    std::vector<double> p, T, bearing;
    std::vector<uint8_t> bad, observes;
    std::vector<int32_t> found, ns, slots, level;
    std::vector<float> px;
    std::vector<int64_t> off;
    bool open(int K, int S, int P, int stride, dsdtm_slam_ctx* shared = nullptr) {
        if (shared) { ctx = shared; own_ctx = false; }
        else CHECK(dsdtm_slam_create(0, &ctx) == DSDTM_OK);
        CHECK(dsdtm_slam_map_create(ctx, &map) == DSDTM_OK);
        p.resize(3 * (size_t)P); bad.assign((size_t)P, 0); found.resize((size_t)P);
        for (size_t i = 0; i < p.size(); ++i) p[i] = 0.25 * (double)(i % 37);
        for (int i = 0; i < P; ++i) found[(size_t)i] = i % 3;
        bad[1] = 1;                                                             // bad before any call, its observing slots set
        CHECK(dsdtm_slam_points_write(ctx, map, 0, P, p.data(), bad.data(), found.data()) == DSDTM_OK);
        for (int k = 0; k < K; ++k) {
            std::vector<int32_t> s((size_t)S), l((size_t)S);
            std::vector<uint8_t> o((size_t)S);
            std::vector<float> x(2 * (size_t)S, 1.f);
            std::vector<double> b(3 * (size_t)S);
            for (int i = 0; i < S; ++i) {
                s[(size_t)i] = (k * stride + i) % P; o[(size_t)i] = (k + i) % 5 != 0; l[(size_t)i] = i % 4;
                for (int r = 0; r < 3; ++r) b[3 * (size_t)i + (size_t)r] = 0.001 * (k * 100 + i) + r;
            }
            double Tk[12];
            memcpy(Tk, I12, sizeof Tk);
            Tk[3] = 0.5 * k;
            int got = -1;
            CHECK(dsdtm_slam_keyframe_add(ctx, map, Tk, S, s.data(), o.data(), x.data(), l.data(), b.data(), &got) == DSDTM_OK && got == k);
            off.push_back((int64_t)slots.size()); ns.push_back(S); T.insert(T.end(), Tk, Tk + 12);
            slots.insert(slots.end(), s.begin(), s.end()); observes.insert(observes.end(), o.begin(), o.end()); px.insert(px.end(), x.begin(), x.end());
            level.insert(level.end(), l.begin(), l.end()); bearing.insert(bearing.end(), b.begin(), b.end());
        }
        return true;
    }
    DSDTM::TrackCommitMap writable() {
        DSDTM::TrackCommitMap m;
        m.n_points = (int32_t)bad.size(); m.found = found.data(); m.bad = bad.data();
        m.n_slots_total = (int64_t)slots.size(); m.point_of_slot = slots.data(); m.observes = observes.data();
        return m;
    }
    DSDTM::TrackMapArrays arrays() const {
        DSDTM::TrackMapArrays m;
        m.sel.n_points = (int32_t)bad.size(); m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = (int32_t)ns.size(); m.sel.T_kf_w = T.data();
        m.sel.n_slots = ns.data(); m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
        m.found = found.data(); m.observes = observes.data(); m.px_xy = px.data(); m.level = level.data(); m.bearing = bearing.data();
        return m;
    }
    // the device map equals the mirror, found counts included
    bool agrees() {
        CHECK(same());
        return true;
    }
    bool same() {
        const size_t P = bad.size(), K = ns.size(), S = slots.size();
        std::vector<double> rp(3 * P), rT(12 * K), rb(3 * S);
        std::vector<uint8_t> rbad(P), ro(S);
        std::vector<int32_t> rf(P), rn(K), rs(S), rl(S);
        std::vector<int64_t> roff(K);
        std::vector<float> rx(2 * S);
        dsdtm_trackmap_image im{};
        im.point_capacity = (int32_t)P; im.keyframe_capacity = (int32_t)K; im.slot_capacity = (int64_t)S;
        im.p_world = rp.data(); im.bad = rbad.data(); im.found = rf.data(); im.T_kf_w = rT.data(); im.n_slots = rn.data(); im.slot_offset = roff.data();
        im.point_of_slot = rs.data(); im.observes = ro.data(); im.px_xy = rx.data(); im.level = rl.data(); im.bearing = rb.data();
        if (dsdtm_slam_map_read(ctx, map, &im) != DSDTM_OK || im.complete != 1) return false;
        return rp == p && rT == T && rbad == bad && rf == found && rs == slots && ro == observes && rl == level && rb == bearing && rn == ns && roff == off;
    }
    void close() { if (own_ctx) dsdtm_slam_destroy(ctx); ctx = nullptr; }
};

struct Frame {
    World* w;
    std::vector<int32_t> point;
    std::vector<double> norm;
};

// one call on `frames` against track_commit_host on the mirrors, which are updated
static bool commit(dsdtm_slam_ctx* ctx, std::vector<Frame>& frames, int bad_capacity) {
    const size_t n = frames.size();
    std::vector<dsdtm_slam_commit_desc> d(n);
    std::vector<std::vector<int32_t>> after(n);
    for (size_t t = 0; t < n; ++t) {
        after[t].assign(frames[t].point.size() + 1, 0);
        fill_a5(after[t].data(), after[t].size() * 4);
        d[t] = {frames[t].w->map, (int32_t)frames[t].point.size(), 0, frames[t].point.data(), frames[t].norm.data(), t % 2 ? nullptr : after[t].data()};
    }
    std::vector<int32_t> bad_points(n * (size_t)bad_capacity + 1);
    fill_a5(bad_points.data(), bad_points.size() * 4);
    std::vector<dsdtm_slam_commit_result> res(n);
    CHECK(dsdtm_slam_track_commit(ctx, THR, (int)n, d.data(), bad_capacity, bad_points.data(), res.data()) == DSDTM_OK);
    for (size_t t = 0; t < n; ++t) {
        const DSDTM::TrackCommitHost h = DSDTM::track_commit_host(frames[t].w->writable(), THR, d[t].n_matches, frames[t].point.data(), frames[t].norm.data());
        const int32_t n_bad = (int32_t)h.bad_points.size();
        CHECK(res[t].n_erased == h.n_erased && res[t].n_bad == n_bad && res[t].overflow_bad == (n_bad > bad_capacity) && res[t].reserved == 0);
        const size_t w = (size_t)std::min(n_bad, bad_capacity);
        CHECK(w == 0 || memcmp(bad_points.data() + t * (size_t)bad_capacity, h.bad_points.data(), w * 4) == 0);
        CHECK(all_a5(bad_points.data() + t * (size_t)bad_capacity + w, ((size_t)bad_capacity - w) * 4));
        if (d[t].found_after) CHECK((h.found_after.empty() || memcmp(after[t].data(), h.found_after.data(), h.found_after.size() * 4) == 0) && all_a5(after[t].data() + h.found_after.size(), 4));
    }
    CHECK(all_a5(bad_points.data() + n * (size_t)bad_capacity, 4));
    return true;
}

static bool commits_and_growth() {
    World a, b;
    CHECK(a.open(8, 24, 60, 7) && a.agrees());
    CHECK(b.open(3, 10, 20, 3, a.ctx) && b.agrees());
    // one frame; a point bad before the call (1) among the matches; points 0, 3, 6 (found 0) go bad
    std::vector<Frame> one = {{&a, {0, 1, 2, 3, 4, 6}, {1.0, 1.0, 1.0, 1.0, 0.25, 0.75}}};
    CHECK(commit(a.ctx, one, 8) && a.agrees() && a.bad[0] == 1 && a.bad[3] == 1 && a.bad[2] == 0);
    // two maps, descs interleaved, a shared point (9: found 0 -> bad through the first, incremented only by the later ones), a lost frame
    std::vector<Frame> mixed = {{&a, {9, 10}, {1.0, 0.0}}, {&b, {9, 0, 5}, {1.0, 1.0, 0.5}}, {&a, {10, 9, 12}, {1.0, 1.0, 1.0}}, {&b, {}, {}}, {&a, {9}, {1.0}},
                                {&b, {0, 9}, {std::nan(""), 1.0}}};
    CHECK(commit(a.ctx, mixed, 1) && a.agrees() && b.agrees() && a.bad[9] == 1 && a.found[9] == 2);
    // 256 matches and a bad_capacity of 0 with bad_points NULL
    World big;
    CHECK(big.open(16, 64, 300, 11, a.ctx));
    Frame f{&big, {}, {}};
    for (int i = 0; i < 256; ++i) { f.point.push_back(299 - i); f.norm.push_back(i % 2 ? 1.0 : 0.0); }
    std::vector<Frame> full = {f};
    CHECK(commit(a.ctx, full, 256) && big.agrees());
    dsdtm_slam_commit_desc d = {big.map, 256, 0, f.point.data(), f.norm.data(), nullptr};
    dsdtm_slam_commit_result r;
    CHECK(dsdtm_slam_track_commit(a.ctx, THR, 1, &d, 0, nullptr, &r) == DSDTM_OK);
    (void)DSDTM::track_commit_host(big.writable(), THR, 256, f.point.data(), f.norm.data());
    CHECK(big.agrees() && dsdtm_slam_track_commit(a.ctx, THR, 0, nullptr, 0, nullptr, nullptr) == DSDTM_OK);
    // 1024 descs on one map: both staging blocks grow
    std::vector<Frame> many(1024, Frame{&big, {}, {}});
    for (int t = 0; t < 1024; ++t)
        for (int i = 0; i < 200; ++i) { many[(size_t)t].point.push_back((t + i) % 300); many[(size_t)t].norm.push_back((t + i) % 3 ? 0.0 : 1.0); }
    const long m0 = fake_hip_calls("hipMalloc");
    CHECK(commit(a.ctx, many, 4) && big.agrees() && fake_hip_calls("hipMalloc") > m0);
    // the mapping thread's entries under their dsdtm_slam_* names, on the map the commits left
    std::vector<int32_t> k(32), wt(32);
    dsdtm_mapping_cov_desc cd = {a.map, 3, 32, k.data(), wt.data()};
    dsdtm_mapping_cov_result cr;
    CHECK(dsdtm_slam_covisibility(a.ctx, 1, &cd, &cr) == DSDTM_OK);
    const DSDTM::CovisibilityHost c = DSDTM::update_connection_host(a.arrays(), 3);
    CHECK(cr.n_cov == (int32_t)c.cov_kf.size() && cr.n_connected == c.n_connected && (c.cov_kf.empty() || memcmp(k.data(), c.cov_kf.data(), c.cov_kf.size() * 4) == 0));
    a.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool validation() {
    World w;
    CHECK(w.open(6, 12, 30, 5));
    dsdtm_slam_ctx* other = nullptr;
    dsdtm_trackmap* foreign = nullptr;
    CHECK(dsdtm_slam_create(0, &other) == DSDTM_OK && dsdtm_slam_map_create(other, &foreign) == DSDTM_OK);
    const int32_t pts[3] = {2, 3, 4}, twice[3] = {2, 3, 2}, far[3] = {2, 30, 4}, neg[3] = {-1, 3, 4};
    const double norms[3] = {1.0, 1.0, 1.0};
    std::vector<int32_t> many(257, 0);
    std::vector<double> many_norms(257, 0.0);
    for (int i = 0; i < 257; ++i) many[(size_t)i] = i % 30;
    int32_t after[2][3], bad_points[2 * 4];
    dsdtm_slam_commit_result res[2];
    fill_a5(after, sizeof after); fill_a5(bad_points, sizeof bad_points); fill_a5(res, sizeof res);
    const long launches = fake_slam_launches();
    auto untouched = [&]() { return all_a5(after, sizeof after) && all_a5(bad_points, sizeof bad_points) && all_a5(res, sizeof res) && fake_slam_launches() == launches && w.agrees(); };
    auto refuse = [&](dsdtm_slam_commit_desc bad, const char* needle) {
        dsdtm_slam_commit_desc d[2] = {{w.map, 3, 0, pts, norms, after[0]}, bad};
        return named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 2, d, 4, bad_points, res), needle) && strstr(dsdtm_slam_last_error(w.ctx), "desc 1") && untouched();
    };
    CHECK(refuse({nullptr, 3, 0, pts, norms, after[1]}, "map is NULL") && refuse({foreign, 3, 0, pts, norms, after[1]}, "not a map of this context"));
    CHECK(refuse({w.map, -1, 0, pts, norms, after[1]}, "n_matches") && refuse({w.map, 257, 0, many.data(), many_norms.data(), nullptr}, "n_matches"));
    CHECK(refuse({w.map, 3, 0, nullptr, norms, after[1]}, "point is NULL") && refuse({w.map, 3, 0, pts, nullptr, after[1]}, "residual_norm is NULL"));
    CHECK(refuse({w.map, 3, 0, far, norms, after[1]}, "point[1] = 30") && refuse({w.map, 3, 0, neg, norms, after[1]}, "point[0] = -1"));
    CHECK(refuse({w.map, 3, 0, twice, norms, after[1]}, "point 2 occurs twice"));
    dsdtm_slam_commit_desc good[2] = {{w.map, 3, 0, pts, norms, after[0]}, {w.map, 3, 0, pts, norms, after[1]}};
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, -1, good, 4, bad_points, res), "outside") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 1025, good, 4, bad_points, res), "outside") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, std::nan(""), 2, good, 4, bad_points, res), "not finite") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, std::numeric_limits<double>::infinity(), 2, good, 4, bad_points, res), "not finite") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 2, good, -1, bad_points, res), "bad_capacity") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 2, nullptr, 4, bad_points, res), "descs is NULL") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 2, good, 4, nullptr, res), "bad_points is NULL") && untouched());
    CHECK(named_err(w.ctx, dsdtm_slam_track_commit(w.ctx, THR, 2, good, 4, bad_points, nullptr), "results is NULL") && untouched());
    CHECK(dsdtm_slam_track_commit(nullptr, THR, 2, good, 4, bad_points, res) == DSDTM_ERR_INVALID && untouched());
    // n == 0: DSDTM_OK with nothing done, whatever the other arguments are
    CHECK(dsdtm_slam_track_commit(w.ctx, std::nan(""), 0, nullptr, -1, nullptr, nullptr) == DSDTM_OK && dsdtm_slam_track_commit(w.ctx, THR, 0, nullptr, 0, nullptr, nullptr) == DSDTM_OK && untouched());
    dsdtm_slam_destroy(other);
    w.close();
    CHECK(fake_hip_errors().empty());
    return true;
}

// every HIP call and the launch on the way of the entry failing once: DSDTM_ERR_HIP, the outputs untouched, the map's bookkeeping and
// (the launch is one step here) the map itself as they were, the context usable
static bool hip_failures() {
    for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize", "hipMalloc", "hipHostMalloc", "hipSetDevice", "launch"})
        for (long nth = 1; nth <= 4; ++nth) {
            World w;
            CHECK(w.open(6, 12, 30, 5));
            const bool launch = strcmp(api, "launch") == 0;
            std::vector<Frame> frames = {{&w, {0, 3, 4, 1}, {1.0, 1.0, 1.0, 1.0}}, {&w, {3, 6}, {1.0, 1.0}}};
            dsdtm_slam_commit_desc d[2] = {{w.map, 4, 0, frames[0].point.data(), frames[0].norm.data(), nullptr}, {w.map, 2, 0, frames[1].point.data(), frames[1].norm.data(), nullptr}};
            int32_t bad_points[8];
            dsdtm_slam_commit_result res[2];
            fill_a5(bad_points, sizeof bad_points); fill_a5(res, sizeof res);
            if (launch) fake_slam_fail(nth); else fake_hip_fail(api, nth);
            const int rc = dsdtm_slam_track_commit(w.ctx, THR, 2, d, 4, bad_points, res);
            fake_slam_fail(0);
            if (!launch) fake_hip_fail(api, 0);
            if (rc != DSDTM_OK) {
                CHECK(rc == DSDTM_ERR_HIP && strlen(dsdtm_slam_last_error(w.ctx)) > 0 && all_a5(bad_points, sizeof bad_points) && all_a5(res, sizeof res));
                dsdtm_trackmap_image im{};
                CHECK(dsdtm_slam_map_read(w.ctx, w.map, &im) == DSDTM_OK && im.n_points == 30 && im.n_keyframes == 6 && im.n_slots_total == 72);
                // a failure in front of the launch, or of the launch itself, has written nothing; behind it (the read-back, the wait) the
                // whole commit is in the map: never a part of it
                if (launch) CHECK(w.same());
                if (!w.same()) for (Frame& f : frames) (void)DSDTM::track_commit_host(w.writable(), THR, (int32_t)f.point.size(), f.point.data(), f.norm.data());
            } else {
                for (Frame& f : frames) (void)DSDTM::track_commit_host(w.writable(), THR, (int32_t)f.point.size(), f.point.data(), f.norm.data());
            }
            CHECK(w.agrees());
            std::vector<Frame> next = {{&w, {7, 8, 9}, {1.0, 0.0, 1.0}}};
            CHECK(commit(w.ctx, next, 4) && w.agrees());             // the context is usable whatever happened
            w.close();
            CHECK(fake_hip_pending() == 0);
        }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// ---- dsdtm_slam_need_keyframes. The fake decision kernel (tests/fake_hip_keyframe) answers with checksums of the blob it is handed:
// the same checksums of gather_keyframe_desc_host's arrays say that the gather's output reached it whole, at the right offsets.
static const dsdtm_camera CAMERA = {512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
static const dsdtm_keyframe_params PRM = {30, 50, 31, 0, 40.0, 0.1, 0.1};

static bool verdict_is_checksum(const dsdtm_keyframe_verdict& v, const DSDTM::KeyframeDescHost& h) {
    auto sum = [](const std::vector<double>& a) { double s = 0; for (double x : a) s += x; return s; };
    auto sum8 = [](const std::vector<uint8_t>& a) { double s = 0; for (uint8_t x : a) s += x; return s; };
    CHECK(v.need == h.n_valid && v.reason == PRM.px_samples && v.n_px == (int32_t)h.kf_bad.size() && v.n_depth == (int32_t)h.cur_bad.size() && v.svo_kf == (int32_t)(h.local_kf_centre.size() / 3));
    CHECK(v.median_px == sum(h.kf_p_world) && v.median_depth == sum(h.cur_p_world) && v.min_depth == sum8(h.cur_bad) + 1000.0 * sum8(h.kf_bad) && v.trans == sum(h.local_kf_centre));
    CHECK(v.rot == h.T_cur_w[3] + h.T_kf_w[11] + (double)CAMERA.fx);
    return true;
}

static bool keyframes_and_validation() {
    World a, b;
    CHECK(a.open(8, 24, 60, 7) && b.open(3, 10, 20, 3, a.ctx));
    // slots that are -1 and a point that is bad in the last keyframe's list
    std::vector<int32_t> s(a.slots.begin() + 24 * 5, a.slots.begin() + 24 * 6);
    std::vector<uint8_t> o(a.observes.begin() + 24 * 5, a.observes.begin() + 24 * 6);
    for (int i : {0, 7, 23}) { s[(size_t)i] = -1; o[(size_t)i] = 0; }
    CHECK(dsdtm_slam_keyframe_write(a.ctx, a.map, 5, nullptr, 0, 24, s.data(), o.data()) == DSDTM_OK);
    std::copy(s.begin(), s.end(), a.slots.begin() + 24 * 5); std::copy(o.begin(), o.end(), a.observes.begin() + 24 * 5);
    double T[12];
    memcpy(T, I12, sizeof T);
    T[3] = 0.25; T[7] = -0.5;
    const std::vector<int32_t> cur = {4, 1, 59, 0, 33}, lk = {7, 0, 3}, none;
    std::vector<int32_t> full_cur;
    for (int i = 0; i < DSDTM_KF_MAX_POINTS; ++i) full_cur.push_back(i % 60);
    std::vector<int32_t> full_lk;
    for (int i = 0; i < DSDTM_KF_MAX_LOCAL_KF; ++i) full_lk.push_back(i % 8);
    dsdtm_slam_keyframe_desc d[4] = {{a.map, T, 41, 5, cur.data(), 5, 3, lk.data()}, {b.map, T, 7, 0, nullptr, 2, 0, nullptr},
                                     {a.map, T, 99, DSDTM_KF_MAX_POINTS, full_cur.data(), 0, DSDTM_KF_MAX_LOCAL_KF, full_lk.data()}, {b.map, T, 3, 1, cur.data() + 3, 0, 1, lk.data() + 1}};
    dsdtm_keyframe_verdict v[5];
    fill_a5(v, sizeof v);
    CHECK(dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &PRM, 4, d, v) == DSDTM_OK && all_a5(&v[4], sizeof v[4]));
    const DSDTM::TrackMapArrays ma = a.arrays(), mb = b.arrays();
    for (int t = 0; t < 4; ++t) {
        const DSDTM::KeyframeDescHost h = DSDTM::gather_keyframe_desc_host(d[t].map == a.map ? ma : mb, T, d[t].n_valid, d[t].n_cur_points, d[t].cur_point, d[t].kf, d[t].n_local_kf, d[t].local_kf);
        CHECK(verdict_is_checksum(v[t], h));
        if (t == 0) CHECK(h.kf_bad.size() == 21 && h.local_kf_centre[0] == -3.5 && h.cur_bad[1] == 1);
    }
    CHECK(a.agrees() && b.agrees());                                        // the entry reads the map only
    // refusals: verdicts untouched, nothing launched
    dsdtm_slam_ctx* other = nullptr;
    dsdtm_trackmap* foreign = nullptr;
    CHECK(dsdtm_slam_create(0, &other) == DSDTM_OK && dsdtm_slam_map_create(other, &foreign) == DSDTM_OK);
    fill_a5(v, sizeof v);
    const long launches = fake_slam_launches();
    double Tnan[12];
    memcpy(Tnan, T, sizeof T);
    Tnan[6] = std::nan("");
    const int32_t far_point[2] = {0, 60}, neg_point[1] = {-1}, far_kf[1] = {8};
    auto refuse = [&](dsdtm_slam_keyframe_desc bad, const char* needle) {
        dsdtm_slam_keyframe_desc dd[2] = {d[0], bad};
        return named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &PRM, 2, dd, v), needle) && strstr(dsdtm_slam_last_error(a.ctx), "tracker 1") && all_a5(v, sizeof v) &&
               fake_slam_launches() == launches;
    };
    CHECK(refuse({nullptr, T, 1, 0, nullptr, 0, 0, nullptr}, "map is NULL") && refuse({foreign, T, 1, 0, nullptr, 0, 0, nullptr}, "not a map of this context"));
    CHECK(refuse({a.map, nullptr, 1, 0, nullptr, 0, 0, nullptr}, "T_cur_w is NULL") && refuse({a.map, Tnan, 1, 0, nullptr, 0, 0, nullptr}, "T_cur_w is not finite"));
    CHECK(refuse({a.map, T, 1, -1, nullptr, 0, 0, nullptr}, "n_cur_points") && refuse({a.map, T, 1, DSDTM_KF_MAX_POINTS + 1, full_cur.data(), 0, 0, nullptr}, "n_cur_points"));
    CHECK(refuse({a.map, T, 1, 0, nullptr, 0, DSDTM_KF_MAX_LOCAL_KF + 1, full_lk.data()}, "n_local_kf") && refuse({a.map, T, 1, 2, nullptr, 0, 0, nullptr}, "cur_point is NULL"));
    CHECK(refuse({a.map, T, 1, 0, nullptr, 0, 1, nullptr}, "local_kf is NULL") && refuse({a.map, T, 1, 0, nullptr, 8, 0, nullptr}, "kf is not") && refuse({a.map, T, 1, 0, nullptr, -1, 0, nullptr}, "kf is not"));
    CHECK(refuse({a.map, T, 1, 2, far_point, 0, 0, nullptr}, "cur_point[1] = 60") && refuse({a.map, T, 1, 1, neg_point, 0, 0, nullptr}, "cur_point[0] = -1") &&
          refuse({a.map, T, 1, 0, nullptr, 0, 1, far_kf}, "local_kf[0] = 8"));
    dsdtm_keyframe_params odd = PRM;
    odd.px_samples = 65;
    CHECK(named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &odd, 1, d, v), "px_samples") && named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &PRM, 1025, d, v), "outside"));
    CHECK(named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, nullptr, &PRM, 1, d, v), "cam is NULL") && named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, nullptr, 1, d, v), "params is NULL"));
    CHECK(named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &PRM, 1, nullptr, v), "descs is NULL") && named_err(a.ctx, dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &PRM, 1, d, nullptr), "verdicts is NULL"));
    CHECK(dsdtm_slam_need_keyframes(nullptr, &CAMERA, &PRM, 1, d, v) == DSDTM_ERR_INVALID && dsdtm_slam_need_keyframes(a.ctx, &CAMERA, &odd, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(all_a5(v, sizeof v) && fake_slam_launches() == launches && a.agrees());
    dsdtm_slam_destroy(other);
    a.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every HIP call and either launch on the way of dsdtm_slam_need_keyframes failing once: DSDTM_ERR_HIP, the verdicts untouched, the map
// as it was (the entry only reads it), the context usable
static bool keyframe_hip_failures() {
    for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize", "hipMalloc", "hipHostMalloc", "hipSetDevice", "gather", "decide"})
        for (long nth = 1; nth <= 4; ++nth) {
            World w;
            CHECK(w.open(6, 12, 30, 5));
            const std::vector<int32_t> cur = {4, 1, 29}, lk = {5, 0};
            dsdtm_slam_keyframe_desc d = {w.map, I12, 12, 3, cur.data(), 2, 2, lk.data()};
            dsdtm_keyframe_verdict v;
            fill_a5(&v, sizeof v);
            const bool gather = strcmp(api, "gather") == 0, decide = strcmp(api, "decide") == 0;
            if (gather) fake_slam_fail(nth); else if (decide) fake_keyframe_fail(nth); else fake_hip_fail(api, nth);
            const int rc = dsdtm_slam_need_keyframes(w.ctx, &CAMERA, &PRM, 1, &d, &v);
            fake_slam_fail(0); fake_keyframe_fail(0);
            if (!gather && !decide) fake_hip_fail(api, 0);
            if (rc != DSDTM_OK) CHECK(rc == DSDTM_ERR_HIP && strlen(dsdtm_slam_last_error(w.ctx)) > 0 && all_a5(&v, sizeof v));
            CHECK(w.agrees());
            CHECK(dsdtm_slam_need_keyframes(w.ctx, &CAMERA, &PRM, 1, &d, &v) == DSDTM_OK);
            const DSDTM::KeyframeDescHost h = DSDTM::gather_keyframe_desc_host(w.arrays(), I12, 12, 3, cur.data(), 2, 2, lk.data());
            CHECK(verdict_is_checksum(v, h));
            std::vector<Frame> next = {{&w, {7, 8, 9}, {1.0, 0.0, 1.0}}};
            CHECK(commit(w.ctx, next, 4) && w.agrees());
            w.close();
            CHECK(fake_hip_pending() == 0);
        }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_slam", dsdtm_slam_create, dsdtm_slam_destroy, dsdtm_slam_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"commits_and_growth", commits_and_growth}, {"validation", validation}, {"hip_failures", hip_failures},
                                                      {"keyframes_and_validation", keyframes_and_validation}, {"keyframe_hip_failures", keyframe_hip_failures},
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
