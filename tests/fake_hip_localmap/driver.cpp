// libdsdtm_amd_localmap.so's host side (dsdtm_amd/csrc/localmap_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified):
// the resident map and its updates (staging ring, growth, retired arrays), the checks, the packing of a select, every failure path —
// under ASan/UBSan/LSan. The launches are the fakes of tests/fake_hip_localmap/fake_localmap.cpp. Test infrastructure
// (tests/test_local_map_fake_hip_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_localmap.h"
#include "../../dsdtm_amd/host/dsdtm_localmap_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_localmap.h"
#include "localmap.h"

static const dsdtm_camera CAM{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
static const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// the host's mirror of a map, and the updates applied to both
struct Mirror {
    std::vector<double> p, T;
    std::vector<uint8_t> bad;
    std::vector<int32_t> ns, slots;
    std::vector<int64_t> off;
    unsigned rng = 12345;
    unsigned next() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }
    int P() const { return (int)bad.size(); }
    int K() const { return (int)ns.size(); }
    DSDTM::LocalMapArrays arrays() const {
        DSDTM::LocalMapArrays m;
        m.n_points = P(); m.p_world = p.data(); m.bad = bad.data(); m.n_keyframes = K(); m.T_kf_w = T.data(); m.n_slots = ns.data();
        m.slot_offset = off.data(); m.point_of_slot = slots.data();
        return m;
    }
};

// points and keyframes drawn by the mirror, written to both; returns false on any mismatch
struct World {
    dsdtm_localmap_ctx* ctx = nullptr;
    dsdtm_localmap* map = nullptr;
    Mirror m;
    bool points(int n) {
        std::vector<double> x(3 * (size_t)n);
        std::vector<uint8_t> b((size_t)n);
        for (int i = 0; i < n; ++i) {
            x[3 * (size_t)i] = (double)(m.next() % 200) / 100.0 - 1.0; x[3 * (size_t)i + 1] = (double)(m.next() % 100) / 100.0 - 0.5;
            x[3 * (size_t)i + 2] = (double)(m.next() % 500) / 100.0 - 1.0; b[(size_t)i] = m.next() % 10 == 0;
        }
        std::vector<double> xs = x;
        std::vector<uint8_t> bs = b;
        CHECK(dsdtm_localmap_points_write(ctx, map, m.P(), n, xs.data(), bs.data()) == DSDTM_OK);
        std::fill(xs.begin(), xs.end(), -99.0); std::fill(bs.begin(), bs.end(), 77);      // the caller's buffers are free at once
        m.p.insert(m.p.end(), x.begin(), x.end()); m.bad.insert(m.bad.end(), b.begin(), b.end());
        return true;
    }
    std::vector<int32_t> draw_slots(int n) {
        std::vector<int32_t> s((size_t)n);
        for (auto& v : s) v = m.P() == 0 || m.next() % 5 == 0 ? -1 : (int32_t)(m.next() % (unsigned)m.P());
        return s;
    }
    bool keyframe(int n_slots) {
        std::vector<int32_t> s = draw_slots(n_slots);
        double T[12];
        memcpy(T, I12, sizeof T);
        T[3] = (double)(m.next() % 16) * 0.25; T[11] = (double)(m.next() % 4) * 0.5;
        std::vector<int32_t> sc = s;
        double Tc[12];
        memcpy(Tc, T, sizeof T);
        int k = -1;
        CHECK(dsdtm_localmap_keyframe_add(ctx, map, Tc, n_slots, sc.data(), &k) == DSDTM_OK && k == m.K());
        std::fill(sc.begin(), sc.end(), 555); Tc[3] = -1e9;
        m.off.push_back((int64_t)m.slots.size()); m.ns.push_back(n_slots);
        m.slots.insert(m.slots.end(), s.begin(), s.end()); m.T.insert(m.T.end(), T, T + 12);
        return true;
    }
    // the device map equals the mirror (map_read), and a select on it equals the host function on the mirror
    bool agrees(int n_local = 6) {
        dsdtm_localmap_image im{};
        CHECK(dsdtm_localmap_map_read(ctx, map, &im) == DSDTM_OK && im.complete == (m.P() == 0 && m.K() == 0));
        CHECK(im.n_points == m.P() && im.n_keyframes == m.K() && im.n_slots_total == (int64_t)m.slots.size());
        std::vector<double> p(m.p.size() + 1), T(m.T.size() + 1);
        std::vector<uint8_t> bad(m.bad.size() + 1);
        std::vector<int32_t> ns(m.ns.size() + 1), slots(m.slots.size() + 1);
        std::vector<int64_t> off(m.off.size() + 1);
        im.point_capacity = m.P(); im.keyframe_capacity = m.K(); im.slot_capacity = (int64_t)m.slots.size();
        im.p_world = p.data(); im.bad = bad.data(); im.T_kf_w = T.data(); im.n_slots = ns.data(); im.slot_offset = off.data(); im.point_of_slot = slots.data();
        CHECK(dsdtm_localmap_map_read(ctx, map, &im) == DSDTM_OK && im.complete == 1);
        p.pop_back(); T.pop_back(); bad.pop_back(); ns.pop_back(); slots.pop_back(); off.pop_back();
        CHECK(p == m.p && T == m.T && bad == m.bad && ns == m.ns && slots == m.slots && off == m.off);
        const int cap = 64;
        std::vector<int32_t> kf((size_t)n_local), pt(cap), pk(cap), kf2((size_t)n_local), pt2(cap), pk2(cap);
        std::vector<double> kd((size_t)n_local), kd2((size_t)n_local);
        fill_a5(kf.data(), kf.size() * 4); fill_a5(pt.data(), cap * 4); fill_a5(pk.data(), cap * 4); fill_a5(kd.data(), kd.size() * 8);
        kf2 = kf; pt2 = pt; pk2 = pk; kd2 = kd;
        dsdtm_localmap_params prm{n_local, 0};
        dsdtm_localmap_desc d{};
        d.map = map; d.T_cur_w = I12; d.kf = kf.data(); d.kf_dist = kd.data(); d.point_capacity = cap; d.point = pt.data(); d.point_kf = pk.data();
        dsdtm_localmap_result r{}, r2{};
        CHECK(dsdtm_localmap_select(ctx, &CAM, &prm, 1, &d, &r) == DSDTM_OK);
        DSDTM::select_local_map_host(CAM, prm, m.arrays(), I12, kf2.data(), kd2.data(), cap, pt2.data(), pk2.data(), &r2);
        CHECK(memcmp(&r, &r2, sizeof r) == 0 && kf == kf2 && pt == pt2 && pk == pk2 && memcmp(kd.data(), kd2.data(), kd.size() * 8) == 0);
        return true;
    }
    bool open() {
        CHECK(dsdtm_localmap_create(0, &ctx) == DSDTM_OK && dsdtm_localmap_map_create(ctx, &map) == DSDTM_OK);
        return true;
    }
    void close() { dsdtm_localmap_map_destroy(ctx, map); dsdtm_localmap_destroy(ctx); ctx = nullptr; map = nullptr; }
};

// the life of a map: many updates with no wait between them (the pinned ring), growth of all three arrays, rewrites
static bool updates_and_growth() {
    World w;
    CHECK(w.open() && w.agrees());
    CHECK(w.points(1) && w.points(63) && w.points(300) && w.agrees());
    CHECK(w.keyframe(0) && w.keyframe(1) && w.keyframe(300) && w.agrees());
    const long waits = fake_hip_calls("hipStreamSynchronize"), applied = fake_localmap_apply_launches();
    for (int i = 0; i < 40; ++i) CHECK(w.points(100) && w.keyframe(420));     // across the initial capacities; the library waits for nothing
    CHECK(fake_localmap_apply_launches() == applied + 80);                      // ONE launch per update
    CHECK(fake_hip_calls("hipStreamSynchronize") - waits == 80);                // (the fake launches' own drains, one each: none by the library)
    CHECK(w.m.P() > dsdtm::LM_INITIAL_POINTS && (int64_t)w.m.slots.size() > dsdtm::LM_INITIAL_SLOTS);
    CHECK(w.agrees());
    while (w.m.K() <= dsdtm::LM_INITIAL_KEYFRAMES) CHECK(w.keyframe(3));
    CHECK(w.agrees());
    // more staged bytes than the pinned block holds before anything waits: the ring wraps behind a wait of its own
    for (int i = 0; i < 12; ++i) CHECK(w.points(4000));
    CHECK(w.agrees());
    // rewrites: a pose, slots, pose and slots together, points with flags
    double T[12];
    memcpy(T, I12, sizeof T);
    T[3] = 0.125;
    CHECK(dsdtm_localmap_keyframe_write(w.ctx, w.map, 2, T, 0, 0, nullptr) == DSDTM_OK);
    memcpy(&w.m.T[24], T, sizeof T);
    std::vector<int32_t> s = w.draw_slots(50);
    CHECK(dsdtm_localmap_keyframe_write(w.ctx, w.map, 2, nullptr, 250, 50, s.data()) == DSDTM_OK);
    std::copy(s.begin(), s.end(), w.m.slots.begin() + w.m.off[2] + 250);
    s = w.draw_slots(7);
    T[11] = 3.0;
    CHECK(dsdtm_localmap_keyframe_write(w.ctx, w.map, 5, T, 10, 7, s.data()) == DSDTM_OK);
    memcpy(&w.m.T[60], T, sizeof T);
    std::copy(s.begin(), s.end(), w.m.slots.begin() + w.m.off[5] + 10);
    const double x[6] = {0.5, 0.25, 2.0, -0.5, 0.0, 3.0};
    const uint8_t b[2] = {1, 0};
    CHECK(dsdtm_localmap_points_write(w.ctx, w.map, 17, 2, x, b) == DSDTM_OK);
    std::copy(x, x + 6, w.m.p.begin() + 51); w.m.bad[17] = 1; w.m.bad[18] = 0;
    CHECK(dsdtm_localmap_points_write(w.ctx, w.map, 19, 1, x, nullptr) == DSDTM_OK);      // NULL flags: not bad
    std::copy(x, x + 3, w.m.p.begin() + 57); w.m.bad[19] = 0;
    CHECK(w.agrees() && w.agrees(1) && w.agrees(64));
    w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every refused call names its field and leaves the map and the outputs as they were; nothing is enqueued
static bool validation() {
    World w, other;
    CHECK(w.open() && other.open());
    CHECK(w.points(10) && w.keyframe(4) && w.keyframe(6) && w.agrees());
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const long copies = fake_hip_calls("hipMemcpyAsync"), launches = fake_localmap_apply_launches() + fake_localmap_select_launches();
    auto named = [&](int rc, const char* what) {
        if (rc != DSDTM_ERR_INVALID || !strstr(dsdtm_localmap_last_error(w.ctx), what)) {
            std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_localmap_last_error(w.ctx));
            return false;
        }
        return true;
    };
    double x[6] = {0, 0, 1, 0, 0, 2}, T[12];
    memcpy(T, I12, sizeof T);
    int32_t s[4] = {0, -1, 9, 3};
    int k = -5;
    CHECK(named(dsdtm_localmap_points_write(w.ctx, nullptr, 0, 1, x, nullptr), "map"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, other.map, 0, 1, x, nullptr), "not a map of this context"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, 11, 1, x, nullptr), "gap"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, -1, 1, x, nullptr), "first"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, 0, -1, x, nullptr), "n is"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, 10, 2, nullptr, nullptr), "p_world is NULL"));
    CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, 10, DSDTM_LOCALMAP_MAX_POINTS, x, nullptr), "exceeds"));
    x[4] = inf; CHECK(named(dsdtm_localmap_points_write(w.ctx, w.map, 10, 2, x, nullptr), "p_world is not finite")); x[4] = 0;
    CHECK(dsdtm_localmap_points_write(w.ctx, w.map, 3, 0, nullptr, nullptr) == DSDTM_OK);            // n == 0: nothing
    CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, nullptr, 4, s, &k), "T_kf_w is NULL"));
    CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, 4, nullptr, &k), "point_of_slot is NULL"));
    CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, -1, s, &k), "n_slots"));
    CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, DSDTM_LOCALMAP_MAX_SLOTS + 1, s, &k), "n_slots"));
    s[2] = 10; CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, 4, s, &k), "point_of_slot[2] = 10"));
    s[2] = -2; CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, 4, s, &k), "point_of_slot[2] = -2")); s[2] = 9;
    T[5] = nan; CHECK(named(dsdtm_localmap_keyframe_add(w.ctx, w.map, T, 4, s, &k), "T_kf_w is not finite"));
    CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, 1, T, 0, 0, nullptr), "keyframe 1: T_kf_w is not finite")); T[5] = 1;
    CHECK(k == -5);
    CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, 2, T, 0, 0, nullptr), "keyframe 2"));
    CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, -1, T, 0, 0, nullptr), "keyframe -1"));
    CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, 0, nullptr, 2, 3, s), "keyframe 0: slots [2, 5) outside its 4 slots"));
    CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, 0, nullptr, 0, 2, nullptr), "point_of_slot is NULL"));
    s[1] = 10; CHECK(named(dsdtm_localmap_keyframe_write(w.ctx, w.map, 1, nullptr, 2, 4, s), "keyframe 1: point_of_slot[1] = 10")); s[1] = -1;
    CHECK(dsdtm_localmap_keyframe_write(w.ctx, w.map, 1, nullptr, 0, 0, nullptr) == DSDTM_OK);      // nothing to write
    CHECK(named(dsdtm_localmap_map_read(w.ctx, other.map, nullptr), "map"));
    CHECK(named(dsdtm_localmap_map_read(w.ctx, w.map, nullptr), "out is NULL"));
    CHECK(named(dsdtm_localmap_map_create(w.ctx, nullptr), "out is NULL"));
    // select
    const int n_local = 3, cap = 8;
    struct Out { int32_t kf[3], pt[8], pk[8]; double kd[3]; } out[3];
    dsdtm_localmap_result res[3];
    dsdtm_localmap_desc d[3];
    double Tc[3][12];
    auto reset = [&]() {
        fill_a5(out, sizeof out); fill_a5(res, sizeof res);
        for (int i = 0; i < 3; ++i) {
            memcpy(Tc[i], I12, sizeof I12);
            d[i] = dsdtm_localmap_desc{};
            d[i].map = w.map; d[i].T_cur_w = Tc[i]; d[i].kf = out[i].kf; d[i].kf_dist = out[i].kd; d[i].point_capacity = cap; d[i].point = out[i].pt; d[i].point_kf = out[i].pk;
        }
    };
    dsdtm_localmap_params prm{n_local, 0};
    dsdtm_camera cam = CAM;
    auto sel = [&](const char* what) {
        const int rc = dsdtm_localmap_select(w.ctx, &cam, &prm, 3, d, res);
        const bool ok = named(rc, what) && all_a5(out, sizeof out) && all_a5(res, sizeof res);
        reset(); prm = dsdtm_localmap_params{n_local, 0}; cam = CAM;
        return ok;
    };
    reset();
    d[1].map = nullptr; CHECK(sel("desc 1: map is NULL"));
    d[2].map = other.map; CHECK(sel("desc 2: map is not a map of this context"));
    d[0].T_cur_w = nullptr; CHECK(sel("desc 0: T_cur_w is NULL"));
    d[1].kf = nullptr; CHECK(sel("desc 1: kf is NULL"));
    d[1].kf_dist = nullptr; CHECK(sel("desc 1: kf_dist is NULL"));
    d[2].point = nullptr; CHECK(sel("desc 2: point is NULL"));
    d[2].point_kf = nullptr; CHECK(sel("desc 2: point_kf is NULL"));
    d[2].point_capacity = -1; CHECK(sel("desc 2: point_capacity"));
    d[2].point_capacity = n_local * DSDTM_LOCALMAP_MAX_SLOTS + 1; CHECK(sel("desc 2: point_capacity"));
    Tc[1][11] = nan; CHECK(sel("desc 1: T_cur_w is not finite"));
    Tc[2][0] = -inf; CHECK(sel("desc 2: T_cur_w is not finite"));
    prm.n_local = 0; CHECK(sel("n_local"));
    prm.n_local = DSDTM_LOCALMAP_MAX_LOCAL + 1; CHECK(sel("n_local"));
    prm.boundary = -1; CHECK(sel("boundary"));
    cam.width = 0; CHECK(sel("camera size"));
    cam.height = -480; CHECK(sel("camera size"));
    CHECK(named(dsdtm_localmap_select(w.ctx, nullptr, &prm, 3, d, res), "cam is NULL"));
    CHECK(named(dsdtm_localmap_select(w.ctx, &cam, nullptr, 3, d, res), "params is NULL"));
    CHECK(named(dsdtm_localmap_select(w.ctx, &cam, &prm, 3, nullptr, res), "descs is NULL"));
    CHECK(named(dsdtm_localmap_select(w.ctx, &cam, &prm, 3, d, nullptr), "results is NULL"));
    CHECK(named(dsdtm_localmap_select(w.ctx, &cam, &prm, -1, d, res), "n = -1"));
    CHECK(named(dsdtm_localmap_select(w.ctx, &cam, &prm, DSDTM_LOCALMAP_MAX_DESCS + 1, d, res), "n = 1025"));
    CHECK(dsdtm_localmap_select(w.ctx, &cam, &prm, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(dsdtm_localmap_select(nullptr, &cam, &prm, 3, d, res) == DSDTM_ERR_INVALID && all_a5(res, sizeof res));
    CHECK(fake_hip_calls("hipMemcpyAsync") == copies && fake_localmap_apply_launches() + fake_localmap_select_launches() == launches);
    // capacity 0 with NULL lists is fine, and the three descs of one map answer alike
    d[1].point_capacity = 0; d[1].point = nullptr; d[1].point_kf = nullptr;
    CHECK(dsdtm_localmap_select(w.ctx, &cam, &prm, 3, d, res) == DSDTM_OK);
    CHECK(res[0].n_points == res[1].n_points && res[1].overflow == (res[1].n_points > 0) && memcmp(&res[0], &res[2], sizeof res[0]) == 0);
    CHECK(memcmp(&out[0], &out[2], sizeof out[0]) == 0 && all_a5(out[1].pt, sizeof out[1].pt));
    CHECK(w.agrees() && other.agrees());
    other.close(); w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// a HIP call that fails, at every call site of every entry: an error, the map as it was, the outputs untouched, nothing pending,
// nothing leaked; the context stays usable
static bool hip_failures() {
    const char* apis[] = {"hipMemcpyAsync", "hipStreamSynchronize", "hipMalloc", "hipHostMalloc", "hipSetDevice", "launch"};
    for (int entry = 0; entry < 4; ++entry)
        for (const char* api : apis)
            for (long nth = 1; nth <= 4; ++nth) {
                World w;
                CHECK(w.open());
                if (entry != 0) CHECK(w.points(dsdtm::LM_INITIAL_POINTS - 2) && w.keyframe(300));      // the next update grows an array
                if (entry == 3) CHECK(w.agrees());                                                 // (and the stream is idle)
                const bool launch = !strcmp(api, "launch");
                if (launch) fake_localmap_fail(nth); else fake_hip_fail(api, nth);
                int rc = DSDTM_OK;
                const double x[12] = {0.1, 0.1, 2.0, 0.2, 0.1, 2.0, 0.3, 0.1, 2.0, 0.4, 0.1, 2.0};
                std::vector<int32_t> s(300, 0);
                int k = -5;
                int32_t kf[2], pt[4], pk[4];
                double kd[2];
                dsdtm_localmap_result res;
                fill_a5(kf, sizeof kf); fill_a5(pt, sizeof pt); fill_a5(pk, sizeof pk); fill_a5(kd, sizeof kd); fill_a5(&res, sizeof res);
                if (entry == 0 || entry == 1) rc = dsdtm_localmap_points_write(w.ctx, w.map, w.m.P(), 4, x, nullptr);
                else if (entry == 2) rc = dsdtm_localmap_keyframe_add(w.ctx, w.map, I12, 300, s.data(), &k);
                else {
                    dsdtm_localmap_params prm{2, 0};
                    dsdtm_localmap_desc d{};
                    d.map = w.map; d.T_cur_w = I12; d.kf = kf; d.kf_dist = kd; d.point_capacity = 4; d.point = pt; d.point_kf = pk;
                    rc = dsdtm_localmap_select(w.ctx, &CAM, &prm, 1, &d, &res);
                }
                if (launch) fake_localmap_fail(0); else fake_hip_fail(api, 0);
                if (rc == DSDTM_OK) {            // (fewer than nth calls of this api on the way)
                    if (entry <= 1) { w.m.p.insert(w.m.p.end(), x, x + 12); w.m.bad.insert(w.m.bad.end(), 4, 0); }
                    if (entry == 2) { CHECK(k == w.m.K()); w.m.off.push_back((int64_t)w.m.slots.size()); w.m.ns.push_back(300); w.m.slots.insert(w.m.slots.end(), s.begin(), s.end()); w.m.T.insert(w.m.T.end(), I12, I12 + 12); }
                } else {
                    CHECK(rc == DSDTM_ERR_HIP && strlen(dsdtm_localmap_last_error(w.ctx)) > 0 && k == -5);
                    CHECK(all_a5(kf, sizeof kf) && all_a5(pt, sizeof pt) && all_a5(pk, sizeof pk) && all_a5(kd, sizeof kd) && all_a5(&res, sizeof res));
                }
                CHECK(w.agrees());               // the map as it was (or as updated), and the context usable
                CHECK(w.points(5) && w.keyframe(9) && w.agrees());
                w.close();
                CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0);
            }
    CHECK(fake_hip_errors().empty());
    return true;
}

// every limit at its value, and one over it
static bool limits() {
    World w;
    CHECK(w.open() && w.points(64));
    std::vector<int32_t> s(DSDTM_LOCALMAP_MAX_SLOTS);
    for (size_t i = 0; i < s.size(); ++i) s[i] = (int32_t)(i % 64);
    int k = -1;
    CHECK(dsdtm_localmap_keyframe_add(w.ctx, w.map, I12, DSDTM_LOCALMAP_MAX_SLOTS, s.data(), &k) == DSDTM_OK && k == 0);
    w.m.off.push_back(0); w.m.ns.push_back(DSDTM_LOCALMAP_MAX_SLOTS); w.m.slots = s; w.m.T.assign(I12, I12 + 12);
    CHECK(w.agrees(DSDTM_LOCALMAP_MAX_LOCAL));
    // 1024 descs of one map in one call: one select launch
    const int n = DSDTM_LOCALMAP_MAX_DESCS, n_local = 2;
    std::vector<dsdtm_localmap_desc> d((size_t)n);
    std::vector<dsdtm_localmap_result> res((size_t)n);
    std::vector<int32_t> kf((size_t)n * n_local), pt((size_t)n * 3), pk((size_t)n * 3);
    std::vector<double> kd((size_t)n * n_local), T((size_t)n * 12);
    for (int i = 0; i < n; ++i) {
        memcpy(&T[12 * (size_t)i], I12, sizeof I12);
        T[12 * (size_t)i + 3] = 0.001 * i;
        d[(size_t)i] = dsdtm_localmap_desc{};
        d[(size_t)i].map = w.map; d[(size_t)i].T_cur_w = &T[12 * (size_t)i]; d[(size_t)i].kf = &kf[(size_t)i * n_local]; d[(size_t)i].kf_dist = &kd[(size_t)i * n_local];
        d[(size_t)i].point_capacity = i % 4; d[(size_t)i].point = i % 4 ? &pt[(size_t)i * 3] : nullptr; d[(size_t)i].point_kf = i % 4 ? &pk[(size_t)i * 3] : nullptr;
    }
    dsdtm_localmap_params prm{n_local, 0};
    const long l0 = fake_localmap_select_launches();
    CHECK(dsdtm_localmap_select(w.ctx, &CAM, &prm, n, d.data(), res.data()) == DSDTM_OK && fake_localmap_select_launches() == l0 + 1);
    for (int i = 0; i < n; ++i) CHECK(res[(size_t)i].n_close == 1 && res[(size_t)i].n_kf == 1 && res[(size_t)i].overflow == 1 && kf[(size_t)i * n_local] == 0 && kd[(size_t)i * n_local] == std::fabs(0.001 * i));
    // the largest point_capacity
    prm.n_local = DSDTM_LOCALMAP_MAX_LOCAL;
    const int cap = DSDTM_LOCALMAP_MAX_LOCAL * DSDTM_LOCALMAP_MAX_SLOTS;
    std::vector<int32_t> big((size_t)cap), bigk((size_t)cap), kfl(DSDTM_LOCALMAP_MAX_LOCAL);
    std::vector<double> kdl(DSDTM_LOCALMAP_MAX_LOCAL);
    d[0].kf = kfl.data(); d[0].kf_dist = kdl.data(); d[0].point_capacity = cap; d[0].point = big.data(); d[0].point_kf = bigk.data();
    CHECK(dsdtm_localmap_select(w.ctx, &CAM, &prm, 1, d.data(), res.data()) == DSDTM_OK && res[0].overflow == 0 && res[0].n_points > 0);
    w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_localmap", dsdtm_localmap_create, dsdtm_localmap_destroy, dsdtm_localmap_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"updates_and_growth", updates_and_growth}, {"validation", validation}, {"hip_failures", hip_failures},
                                                      {"limits", limits}, {"create_failures", create_failures}};
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
